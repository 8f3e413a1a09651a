"""No GPU: the host side of the 10-bit YUV 4:2:0 ingest and of sited chroma - the shifted filter table (its sign and size on a ramp), the oracle of
tests/ingest_yuv16_oracle.py pinned to F.interpolate at shift 0, the 10-bit colour matrix, the arguments of RecordingIngest, the ABI entry of
sf_ingest_video_yuv16 and its argument rejection (before the device is touched), and the margin of the pixel bar: the kernel's arithmetic restated in fp32 against
the float64 oracle."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_yuv16_oracle as Y16  # noqa: E402


@pytest.mark.parametrize('n_in, n_out', [(128, 256), (540, 256), (960, 454), (170, 340)])
def test_shift_zero_is_the_table_of_before(n_in, n_out):
    from synchformer_amd.ingest import aa_bicubic_table
    for dtype in (torch.float32, torch.float64):
        f0, w0, t0 = aa_bicubic_table(n_in, n_out, dtype)
        f1, w1, t1 = aa_bicubic_table(n_in, n_out, dtype, shift=0.0)
        assert t0 == t1 and torch.equal(f0, f1) and torch.equal(w0, w1)
    assert not torch.equal(aa_bicubic_table(n_in, n_out)[1], aa_bicubic_table(n_in, n_out, shift=0.25)[1])


def _apply64(first, w, p):
    pad = torch.cat([p, torch.zeros(w.shape[1], dtype=torch.float64)])
    return (w * pad[first.long()[:, None] + torch.arange(w.shape[1])]).sum(1)


@pytest.mark.parametrize('n_in, n_out', [(128, 256), (170, 340)])
def test_shift_moves_a_ramp_by_a_quarter_sample(n_in, n_out):
    """The sign and the size of the shift: on p[k] = k (sample k at coordinate k + 0.5) the unshifted table returns the line itself, scale (i + 0.5) - 0.5, and the
    table with shift=0.25 returns it 0.25 higher - the picture is read a quarter of a source sample further right, which is where a chroma sample co-sited with
    the even luma column sits.  Interior output samples only (the edge rows are clamped), upscaling only (the stretched kernel of a downscale does not reproduce
    lines exactly: 0.012 at 480 -> 454, with or without the shift)."""
    from synchformer_amd.ingest import aa_bicubic_table
    p = torch.arange(n_in, dtype=torch.float64)
    r0 = _apply64(*aa_bicubic_table(n_in, n_out, torch.float64)[:2], p)
    r1 = _apply64(*aa_bicubic_table(n_in, n_out, torch.float64, shift=0.25)[:2], p)
    sl = slice(8, n_out - 8)
    line = n_in / n_out * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5
    print(f'{n_in} -> {n_out}: |unshifted - line| {(r0 - line)[sl].abs().max().item():.2e}, |shifted - unshifted - 0.25| {(r1 - r0 - 0.25)[sl].abs().max().item():.2e}')
    assert (r0 - line)[sl].abs().max().item() <= 1e-12
    assert (r1 - r0 - 0.25)[sl].abs().max().item() <= 1e-12


def test_oracle_at_shift_zero_is_f_interpolate():
    """The oracle itself: its dense float64 filter at shift 0 against ingest_oracle.resize64 (F.interpolate on float64) on all three planes, to 1e-9 of a 10-bit
    level scale of 1023; and against the package's table, entry by entry, with and without the shift."""
    from synchformer_amd.ingest import aa_bicubic_table
    for (H, W), size in (((270, 480), (256, 454)), ((144, 176), (256, 312)), ((360, 202), (456, 256))):
        for p in Y16.random_planes(2, H, W, H + W):
            err = (Y16.resize_dense(p, size) - Y16.resize64(p, size)).abs().max().item()
            print(f'{H} x {W} plane {tuple(p.shape[1:])} -> {size}: max |dense - F.interpolate| {err:.2e}')
            assert err <= 1e-9, err
    for n_in, n_out in ((128, 256), (540, 256), (960, 454), (170, 340)):
        for shift in (0.0, 0.25):
            first, w, taps = aa_bicubic_table(n_in, n_out, torch.float64, shift=shift)
            A = torch.zeros(n_out, n_in + taps, dtype=torch.float64)
            A.scatter_(1, first.long()[:, None] + torch.arange(taps), w)
            assert (A[:, :n_in] - Y16.dense_filter(n_in, n_out, shift)).abs().max().item() <= 1e-14 and float(A[:, n_in:].abs().max()) == 0.0


def test_csc_matrix_10_bit():
    from synchformer_amd.ingest import csc_matrix
    for cs in ('bt601', 'bt709'):
        M8, o8 = csc_matrix(cs, False)
        M10, o10 = csc_matrix(cs, False, bit_depth=10)
        assert M10.dtype == o10.dtype == torch.float64
        assert torch.equal(M10.float(), M8.float() / 4) and torch.equal(o10, 4 * o8) and o10.tolist() == [64.0, 512.0, 512.0]
        Mf, of = csc_matrix(cs, True, bit_depth=10)
        assert of.tolist() == [0.0, 512.0, 512.0]
        white = Mf @ (torch.tensor([1023.0, 512.0, 512.0], dtype=torch.float64) - of)
        assert (white - 255.0).abs().max().item() <= 1e-9, white
        for full in (False, True):                                               # and the oracle's own formula agrees
            M, off = csc_matrix(cs, full, bit_depth=10)
            Mo, oo = Y16.matrix64_10(cs, full)
            assert (M - Mo).abs().max().item() <= 1e-15 and torch.equal(off, oo)
            assert torch.equal(csc_matrix(cs, full, bit_depth=8)[0], csc_matrix(cs, full)[0])
    with pytest.raises(ValueError, match='bit_depth'):
        csc_matrix('bt601', False, bit_depth=12)
    with pytest.raises(ValueError, match='colorspace'):
        csc_matrix('bt2020', False, bit_depth=10)


def test_recording_ingest_chroma_loc_and_csc():
    from synchformer_amd.ingest import PIX_FMTS, RecordingIngest, aa_bicubic_table
    assert PIX_FMTS[:3] == ('rgb24', 'nv12', 'yuv420p') and set(PIX_FMTS[3:]) == {'p010', 'yuv420p10le'}
    cpu = torch.device('cpu')
    luma = ('y_first', 'y_w', 'x_first', 'x_w')
    for pix_fmt in ('nv12', 'yuv420p', 'p010', 'yuv420p10le'):
        c = RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt=pix_fmt)
        d = RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt=pix_fmt, chroma_loc='center')
        le = RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt=pix_fmt, chroma_loc='left')
        tl = RecordingIngest(cpu, 25, (1080, 1920), 48000, pix_fmt=pix_fmt, chroma_loc='topleft')
        assert (c.chroma_loc, le.chroma_loc, tl.chroma_loc) == ('center', 'left', 'topleft')
        for k in luma + ('cy_first', 'cy_w', 'cx_first', 'cx_w', 'csc'):
            assert torch.equal(getattr(c, k), getattr(d, k)), k
        for k in luma + ('cy_first', 'cy_w', 'csc'):                            # 'left' changes only the cx tables
            assert torch.equal(getattr(c, k), getattr(le, k)), k
        assert not torch.equal(c.cx_w, le.cx_w)
        for k in luma + ('csc',):                                                # 'topleft' the cx and the cy tables
            assert torch.equal(getattr(c, k), getattr(tl, k)), k
        assert not torch.equal(c.cy_w, tl.cy_w) and torch.equal(tl.cx_w, le.cx_w) and torch.equal(tl.cx_first, le.cx_first)
        cyf, cyw, _ = aa_bicubic_table(540, 256, shift=0.25)
        cxf, cxw, _ = aa_bicubic_table(960, 454, shift=0.25)
        assert torch.equal(tl.cy_first, cyf[16:240]) and torch.equal(tl.cy_w, cyw[16:240]) and torch.equal(le.cx_first, cxf[115:339]) and torch.equal(le.cx_w, cxw[115:339])
        assert (le.taps_cy, le.taps_cx, tl.taps_cy, tl.taps_cx) == (11, 11, 11, 11)
    # the matrix follows the format's sample scale; an explicit one is used as given
    for cs, full in (('bt601', False), ('bt709', True)):
        M, off = Y16.matrix64_10(cs, full)
        for pix_fmt in Y16.FMTS:
            ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt=pix_fmt, colorspace=cs, full_range=full)
            assert ing.csc.dtype == torch.float32 and ing.csc.device.type == 'cpu' and torch.equal(ing.csc, torch.cat([M.reshape(9), off]).float())
    M2020 = torch.tensor([[0.2851, 0.0, 0.4110], [0.2851, -0.0459, -0.1593], [0.2851, 0.5244, 0.0]], dtype=torch.float64)
    o2020 = torch.tensor([64.0, 512.0, 512.0], dtype=torch.float64)
    for given in ((M2020, o2020), (M2020.tolist(), o2020.tolist()), (M2020.float(), o2020.float())):
        ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='p010', colorspace='bt709', full_range=True, csc=given)
        assert torch.equal(ing.csc, torch.cat([M2020.reshape(9), o2020]).float())
    ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='nv12', csc=(M2020 * 4, o2020 / 4))
    assert torch.equal(ing.csc, torch.cat([(M2020 * 4).reshape(9), o2020 / 4]).float())
    with pytest.raises(ValueError, match='csc'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='p010', csc=(M2020[:2], o2020))


def test_recording_ingest_yuv16_argument_validation():
    from synchformer_amd.ingest import RecordingIngest
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='chroma_loc'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='p010', chroma_loc='bottom')
    with pytest.raises(ValueError, match='chroma_loc'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='nv12', chroma_loc='right')
    with pytest.raises(ValueError, match='chroma_loc'):
        RecordingIngest(cpu, 25, (270, 480), 16000, chroma_loc='left')          # rgb24 has no chroma
    with pytest.raises(ValueError, match='chroma_loc'):
        RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt='rgb24', chroma_loc='topleft')
    for pix_fmt in Y16.FMTS:
        with pytest.raises(ValueError, match='even'):
            RecordingIngest(cpu, 25, (301, 518), 16000, pix_fmt=pix_fmt)
        with pytest.raises(ValueError, match='even'):
            RecordingIngest(cpu, 25, (302, 517), 16000, pix_fmt=pix_fmt)
        with pytest.raises(ValueError, match='channels_last'):
            RecordingIngest(cpu, 25, (270, 480), 16000, channels_last=True, pix_fmt=pix_fmt)
        ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt=pix_fmt)
        with pytest.raises(ValueError, match='raw frames'):                      # 8-bit frames for a 10-bit format
            ing.frames(torch.zeros(4, 405, 480, dtype=torch.uint8), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, 405, 480, dtype=torch.float16), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, 404, 480, dtype=torch.uint16), 0, 1)
    for pix_fmt in ('nv12', 'yuv420p'):                                          # and the reverse
        ing = RecordingIngest(cpu, 25, (270, 480), 16000, pix_fmt=pix_fmt, chroma_loc='left')
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, 405, 480, dtype=torch.uint16), 0, 1)
        with pytest.raises(ValueError, match='raw frames'):
            ing.frames(torch.zeros(4, 405, 480, dtype=torch.int16), 0, 1)


def test_abi_lists_the_yuv16_launcher():
    from synchformer_amd import _lib
    assert _lib.ABI_VERSION >= 17
    assert len(_lib.SIGNATURES['sf_ingest_video_yuv16']) == len(_lib.SIGNATURES['sf_ingest_video_yuv']) + 1 == 28
    for lib in (_lib.load(), _lib.load_ablation()):
        assert hasattr(lib, 'sf_ingest_video_yuv16') and lib.sf_abi_version() >= 17


def test_yuv16_launcher_rejects_bad_arguments_without_gpu():
    from synchformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    v = dict(raw=p, sf=300, sy=20, uo=200, vo=202, csy=20, csx=4, shift=6, n_src=1, H=10, W=10, ft=p, yf=p, yw=p, ty=5, xf=p, xw=p, tx=5, cyf=p, cyw=p, tcy=5,
             cxf=p, cxw=p, tcx=5, csc=p, out=p, T=1)

    def yuv(**kw):
        a = dict(v, **kw)
        return lib.sf_ingest_video_yuv16(a['raw'], a['sf'], a['sy'], a['uo'], a['vo'], a['csy'], a['csx'], a['shift'], a['n_src'], a['H'], a['W'], a['ft'], a['yf'],
                                         a['yw'], a['ty'], a['xf'], a['xw'], a['tx'], a['cyf'], a['cyw'], a['tcy'], a['cxf'], a['cxw'], a['tcx'], a['csc'], a['out'],
                                         a['T'], None)

    for name in ('raw', 'ft', 'yf', 'yw', 'xf', 'xw', 'cyf', 'cyw', 'cxf', 'cxw', 'csc', 'out'):
        assert yuv(**{name: None}) == -1 and b'null pointer' in lib.sf_last_error(), name
    for name, odd in (('sf', 301), ('sy', 21), ('uo', 201), ('vo', 203), ('csy', 21), ('csx', 3)):
        assert yuv(**{name: odd}) == -1 and b'odd' in lib.sf_last_error(), name
        assert yuv(**{name: odd, 'T': 0}) == -1, name
    assert yuv(raw=p + 1) == -1 and b'2-byte aligned' in lib.sf_last_error()
    for shift in (7, -1, 16):
        assert yuv(shift=shift) == -1 and b'shift' in lib.sf_last_error(), shift
    for shift in range(7):
        assert yuv(shift=shift, T=0) == 0, shift
    assert yuv(H=11) == -1 and b'even' in lib.sf_last_error()
    assert yuv(W=9) == -1 and b'even' in lib.sf_last_error()
    for name in ('ty', 'tx', 'tcy', 'tcx'):
        assert yuv(**{name: 0}) == -1 and b'out of range' in lib.sf_last_error(), name
        assert yuv(**{name: 36}) == -1 and b'out of range' in lib.sf_last_error(), name
        assert yuv(**{name: 35, 'T': 0}) == 0, name
    assert yuv(out=p + 1) == -1 and b'aligned' in lib.sf_last_error()
    assert yuv(csx=0) == -1 and b'stride' in lib.sf_last_error()
    assert yuv(sy=-2) == -1 and b'stride' in lib.sf_last_error()
    assert yuv(W=70000) == -1 and b'too wide' in lib.sf_last_error()
    assert yuv(W=5200, tx=35) == -1 and b'too wide' in lib.sf_last_error()
    assert yuv(W=5100, tcx=35) == -1 and b"too wide" in lib.sf_last_error() and b"chroma" in lib.sf_last_error()    # luma fits, chroma does not
    assert yuv(T=-1) == -1 and yuv(T=65536) == -1 and yuv(H=0) == -1
    assert yuv(T=0) == 0                                                         # nothing to do: returns before any launch


def test_ops_ingest_video_yuv16_refuses_before_the_device():
    from synchformer_amd import ops
    from synchformer_amd.ingest import RecordingIngest
    ing = RecordingIngest(torch.device('cpu'), 25, (270, 480), 16000, pix_fmt='p010')
    tabs = (ing.y_first, ing.y_w, ing.x_first, ing.x_w, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w, ing.csc)
    pick = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match='pix_fmt'):
        ops.ingest_video_yuv16(torch.zeros(1, 405, 480, dtype=torch.uint16), 'nv12', pick, *tabs)
    with pytest.raises(ValueError, match='expected uint16'):
        ops.ingest_video_yuv16(torch.zeros(1, 405, 480, dtype=torch.uint8), 'p010', pick, *tabs)
    with pytest.raises(ValueError, match='even H and W'):
        ops.ingest_video_yuv16(torch.zeros(1, 404, 480, dtype=torch.uint16), 'p010', pick, *tabs)
    with pytest.raises(ValueError, match='contiguous rows'):
        ops.ingest_video_yuv16(torch.zeros(1, 405, 512, dtype=torch.uint16)[:, :, :480], 'yuv420p10le', pick, *tabs)
    for dtype in (torch.uint16, torch.int16):
        with pytest.raises(RuntimeError, match='device tensor'):                 # a CPU tensor: no fallback
            ops.ingest_video_yuv16(torch.zeros(1, 405, 480, dtype=dtype), 'p010', pick, *tabs)


@pytest.mark.parametrize('H, W', [(270, 480), (1080, 608), (144, 176), (540, 960)])
def test_fp32_restatement_stays_inside_the_pixel_bar(H, W):
    """The margin the GPU bar leaves, on the 10-bit scale and with sited chroma: the package's tables and matrix evaluated in fp32 on the CPU (horizontal pass
    first, taps ascending - the kernel's order up to its fused multiply-adds) against the float64 oracle on uniform random 10-bit planes.  Measured: at most 1
    level, 6.6e-6 to 2.0e-5 of the pixels differ (asserted: <= 1e-4, a tenth of the bar of check_pixels), 9-28 % of the values lie outside [0, 255] before the
    clamp."""
    from synchformer_amd.ingest import RecordingIngest
    cs, full, loc = Y16.CASES[(H, W)]
    planes = Y16.random_planes(2, H, W, H * 10000 + W)
    Hr, Wr, y0, x0 = Y16.origin(H, W)
    ref, outside = Y16.oracle(planes, (Hr, Wr), y0, x0, *Y16.matrix64_10(cs, full), loc)
    ing = RecordingIngest(torch.device('cpu'), 25, (H, W), 16000, pix_fmt='p010', colorspace=cs, full_range=full, chroma_loc=loc)
    r = [Y16.apply_tables32(planes[0], ing.y_first, ing.y_w, ing.x_first, ing.x_w)] + \
        [Y16.apply_tables32(p, ing.cy_first, ing.cy_w, ing.cx_first, ing.cx_w) for p in planes[1:]]
    m, o = ing.csc[:9].reshape(3, 3), ing.csc[9:]
    pre = torch.einsum('ck,nkyx->ncyx', m, torch.stack([r[0] - o[0], r[1] - o[1], r[2] - o[2]], 1))
    got = pre.round().clamp(0, 255).to(torch.uint8)
    Y16.check_pixels(got, ref, f'{H} x {W} {cs} {"full" if full else "limited"} {loc}: fp32 restatement, {outside:.1%} outside [0, 255] before the clamp')
    assert (got.int() - ref.int()).ne(0).float().mean().item() <= 1e-4
    assert outside > 0, outside
