"""GPU: the kernels every forward pass goes through first - sf_layernorm768, sf_quantize_mxfp8 / sf_layernorm768_mxfp8, sf_broadcast_rows768 / sf_gather_rows768, the patch
gathers (sf_im2col_video / _clips / _tokens, sf_im2col_spec), the token masks and the mel front-end - against the float64 / integer references of
tests/rowops_fwd_oracle.py (tests/test_rowops_fwd_oracle_cpu.py shows that these criteria reject a subtly wrong kernel).

Every output lives in a buffer pre-filled with gemm_oracle.canary, which must survive bit for bit wherever the kernel has no business: rows beyond the last, the pad columns of
a strided output, the rows a map skips, the scale-plane rows beyond `rows`.  Strided operands are column slices (16-byte aligned; a bf16 output at 8 bytes) of wider NaN-filled
buffers.  Every written element is compared.  Row counts cross the kernels' own boundaries (4 rows per 256-thread block: 1, 3, 4, 5, 9) plus one of a few hundred.  No launch
leaves its launcher's contract: the refusals (include/synchformer_hip.h) are asserted from the return code and sf_last_error, with rows = 0 wherever a library without the check
would otherwise launch.

Measured on the MI355X (set SF_ROWOPS_TEST_STATS=<file> to have every check append its figures).  checks = recorded launches (LayerNorm, mel) or test cases of several
launches each (the byte- and bit-exact kernels); worst = the largest err / bar; for the mel front-end also the worst per-frame ||got - ref|| / limit of the tonal families
and the smallest share of computed elements whose bar is under the 5e-3 cap, over the nine cases of MEL_CASES.
  kernel                  output       family                checks     worst   per-frame  share <= cap
  sf_layernorm768         fp32         gauss                     19    0.0469
  sf_layernorm768         fp32 +=      gauss                     21      0.11
  sf_layernorm768         bf16         gauss                     19       0.5
  sf_layernorm768         fp32         offset100                 19    0.0459
  sf_layernorm768         fp32 +=      offset100                 21    0.0465
  sf_layernorm768         bf16         offset100                 19     0.491
  sf_layernorm768         fp32         offset1e4                 18    0.0422
  sf_layernorm768         fp32 +=      offset1e4                 18    0.0422
  sf_layernorm768         bf16         offset1e4                 18    0.0431
  sf_layernorm768         fp32         spike                     18    0.0412
  sf_layernorm768         fp32 +=      spike                     18     0.561
  sf_layernorm768         bf16         spike                     18       0.5
  sf_layernorm768         fp32         scales                    18    0.0429
  sf_layernorm768         fp32 +=      scales                    18     0.912
  sf_layernorm768         bf16         scales                    18       0.5
  sf_layernorm768         fp32         const                     18         0
  sf_layernorm768         fp32 +=      const                     18     0.944
  sf_layernorm768         bf16         const                     18       0.5
  sf_quantize_mxfp8       e4m3 + e8m0  constructed blocks        16     exact
  sf_layernorm768_mxfp8   e4m3 + e8m0  gauss, scales, spike       3     exact
  sf_broadcast_rows768    fp32         bit patterns               4     exact
  sf_gather_rows768       fp32, bf16   bit patterns               3     exact
  sf_im2col_video         bf16         u8 / f16 / bf16 / f32      4     exact
  sf_im2col_video_clips   bf16         u8 / f16 / bf16 / f32      4     exact
  sf_im2col_video_tokens  bf16         u8, f32                    2     exact
  sf_im2col_spec          bf16         4 shapes x n_seg 1, 3      8     exact
  sf_token_mask_video     u8           crafted                    2     exact
  sf_token_mask_spec      u8           4 shapes x n_seg 1, 2      8     exact
  sf_mel_frontend         fp32         noise                      9    0.0166                   1.000
  sf_mel_frontend         fp32         gauss1e-4                  9    0.0356                   1.000
  sf_mel_frontend         fp32         gauss1e3                   9    0.0209                   1.000
  sf_mel_frontend         fp32         impulse0                   9     0.123                   1.000
  sf_mel_frontend         fp32         impulse_last               9     0.351                   1.000
  sf_mel_frontend         fp32         silence                    9     0.123                   1.000
  sf_mel_frontend         fp32         dc                         9    0.0232      0.0293       0.125
  sf_mel_frontend         fp32         tone100                    9    0.0335      0.0148       0.162
  sf_mel_frontend         fp32         tone440                    9     0.027      0.0117       0.185
  sf_mel_frontend         fp32         tone7900                   9    0.0146       0.431       0.017
The plain fp32 LayerNorm rows measure the kernel: 0.04 - 0.05 of the bar on every family, where a one-pass variance would stand at 13 (offset100).  A bf16 output's 0.5 is
its own rounding (half an ulp against a bar of one), the accumulated output's 0.56 - 0.94 the rounding of the final sum where y is small next to the prefill (spike, scales,
const: half an ulp of the sum is up to 2^-24 (|prefill| + |y|), all of its term).  The constant rows come out as beta itself: in this order the mean of 768 equal integers
rounds back to the integer, so the bar's mean term is not drawn on.  Mel: silence and the frames an impulse does not reach sit at log(1e-6), where 0.123 of the bar is
logf and the two roundings behind it; impulse_last's 0.351 is one such frame.  Tones and DC keep 2 - 19 % of their elements under the cap (a pure tone leaves most mel bins
with leakage below the 1e-6 floor, where the worst-case bar is vacuous, up to 0.6); there the per-frame criterion holds the kernel to the emulation, at most 0.06 of the limit
with 128 filters and 0.43 with 40 (tone7900: fewer, wider filters - each sums more leakage bins, whose rounding noise the kernel and the emulation do not share bit for bit).
No kernel needed a fix; the launchers gained the argument checks that test_row_launchers_refuse asserts.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402
import rowops_fwd_oracle as R  # noqa: E402
from test_gemm_gpu import _Out, _place  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F16, U8 = torch.float32, torch.bfloat16, torch.float16, torch.uint8
_STATS_PATH = os.environ.get('SF_ROWOPS_TEST_STATS')
ROWS = (1, 3, 4, 5, 9, 301)
LDS = ((768, 768), (776, 768), (768, 776), (776, 776))
SPEC_SHAPES = ((128, 66), (16, 16), (37, 29), (26, 17))


def _record(kernel, output, family, worst, *more):
    if _STATS_PATH:
        with open(_STATS_PATH, 'a') as f:
            f.write('\t'.join([kernel, output, family, f'{worst:.4g}'] + [f'{m:.4g}' for m in more]) + '\n')


def _off(ld, width=768):
    """Column offset of a strided operand inside its wider buffer: 4 elements (16 bytes of fp32, 8 of bf16) when there is room."""
    return 4 if ld > width else 0


def _refused(lib, rc, text):
    assert rc == -1, rc
    msg = lib.sf_last_error().decode()
    assert text in msg, msg


@pytest.fixture(scope='module')
def lib(gpu):
    from synchformer_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def blocks():
    return R.mx_blocks()


@pytest.fixture(scope='module')
def ln_params(gpu):
    g, b = R.ln_params(4)
    return g, b, g.to(gpu), b.to(gpu)


# =====================================================================================================================================================
# 1. sf_layernorm768
# =====================================================================================================================================================
def _ln_once(gpu, ln_params, family, x, eps, out, ldx, ldy, in_map=None, out_map=None, x_rows=None, out_rows=None):
    """One launch: x (rows, 768) are the LOGICAL rows; they are laid at in_map's physical rows of a NaN buffer, the output is read at out_map's rows."""
    from synchformer_amd import ops
    g, b, gd, bd = ln_params
    rows = x.shape[0]
    src = R.map_rows(in_map, rows)
    xin = torch.full((int(src.max()) + 1 if x_rows is None else x_rows, 768), float('nan'))
    xin[src] = x
    dst = R.map_rows(out_map, rows)
    prefill = 2 * torch.randn(rows, 768, generator=G.gen(rows)) + 0.25 if out == 'acc' else None
    O = _Out(gpu, rows, 768, BF16 if out == 'bf16' else F32, ld=ldy, off=_off(ldy), rows=(int(dst.max()) + 4 if out_rows is None else out_rows), idx=dst, init=prefill)
    ops.layernorm(_place(xin, ldx, _off(ldx), gpu), gd, bd, O.view, eps, rows=rows, in_map=in_map, out_map=out_map, accumulate=out == 'acc')
    ref, bar = R.ln_expected(x, g, b, eps, out == 'bf16', prefill)
    res = R.elem_check(O.get().float(), ref, bar)
    print(f'sf_layernorm768 {out} {family} eps {eps} rows {rows} ld {ldx}/{ldy}: worst err / bar {res["worst"]:.3g}')
    assert res['msg'] is None, f'{out} {family} rows {rows} ld {ldx}/{ldy}: {res["msg"]}'
    _record('sf_layernorm768', out, family, res['worst'])


@pytest.mark.parametrize('eps', R.LN_EPS)
@pytest.mark.parametrize('family', R.LN_FAMILIES)
def test_layernorm(gpu, ln_params, family, eps):
    """fp32, fp32 accumulated onto a non-zero prefill and bf16 outputs at every row count, the strides rotating through ldx, ldy in {768, 776}."""
    i = 0
    for rows in ROWS:
        x = R.ln_input(family, rows, seed=rows)
        for out in ('f32', 'acc', 'bf16'):
            ldx, ldy = LDS[i % 4]
            i += 1
            _ln_once(gpu, ln_params, family, x, eps, out, ldx, ldy)


@pytest.mark.parametrize('family', ('gauss', 'offset100'))
def test_layernorm_row_maps(gpu, ln_params, family):
    """The engine's drop-CLS regroup (one sequence: 1568 patch rows of 1569 -> rows 1 .. 196 of eight 197-row frames; row 0 of each keeps the canary) and the audio
    aggregator's transposing map with accumulate (two sequences: (fi, ti) of rows 2 .. 73 of 74 -> row ti * 13 + 1 + fi of 78; rows ti * 13 keep the canary)."""
    x = R.ln_input(family, 1568, seed=21)
    for out, (ldx, ldy) in (('f32', LDS[3]), ('bf16', LDS[1]), ('acc', LDS[2])):
        _ln_once(gpu, ln_params, family, x, 1e-6, out, ldx, ldy, in_map=(1568, 1568, 1569, 0, 1, 1), out_map=(1568, 196, 8 * 197, 197, 1, 1), x_rows=1569, out_rows=8 * 197 + 2)
    xa = R.ln_input(family, 144, seed=22)
    for ldx, ldy in (LDS[0], LDS[3]):
        _ln_once(gpu, ln_params, family, xa, 1e-12, 'acc', ldx, ldy, in_map=(72, 72, 74, 0, 1, 2), out_map=(72, 6, 78, 1, 13, 1), x_rows=148, out_rows=2 * 78 + 2)


def test_row_launchers_refuse(gpu, lib, ln_params):
    """The contract of the 768-column row launchers: strides that are multiples of 4, 16-byte aligned fp32 pointers, 8-byte aligned bf16 outputs, rows < 2^31 under a row
    map, accumulate only into fp32.  rows = 0 throughout (nothing could launch), except for the row-count refusal, which is sent only after the others have shown that
    this library checks its arguments."""
    from synchformer_amd import ops
    x = torch.zeros(8, 776, device=gpu)
    y = torch.zeros(8, 776, device=gpu)
    yb = torch.zeros(8, 776, device=gpu, dtype=BF16)
    q = torch.zeros(8, 784, device=gpu, dtype=U8)
    sc = torch.zeros(6, 8, 4, device=gpu, dtype=U8)
    _, _, gd, bd = ln_params
    X, Y, YB, GA, BE, Q, SC = (t.data_ptr() for t in (x, y, yb, gd, bd, q, sc))
    ident = (ctypes.c_int64 * 6)(1, 1, 1, 0, 0, 0)
    ln = lambda x_=X, ldx=776, g_=GA, b_=BE, y_=Y, dt=0, ldy=776, acc=0, rows=0, im=None, om=None: \
        lib.sf_layernorm768(x_, ldx, im, g_, b_, y_, dt, ldy, om, acc, rows, 1e-6, None)                                         # noqa: E731
    assert ln() == 0
    _refused(lib, ln(acc=1, y_=YB, dt=1), 'accumulate needs f32')
    _refused(lib, ln(ldx=770), 'multiple of 4')
    _refused(lib, ln(ldy=774), 'multiple of 4')
    for kw in (dict(x_=X + 4), dict(x_=X + 8), dict(g_=GA + 4), dict(b_=BE + 8), dict(y_=Y + 8), dict(y_=YB + 4, dt=1), dict(y_=YB + 2, dt=1)):
        _refused(lib, ln(**kw), 'aligned')
    assert ln(y_=YB + 8, dt=1) == 0                                                    # a bf16 output needs 8 bytes only
    ga = lambda x_=X, ldx=776, y_=Y, dt=0, ldy=776, rows=0, im=None: lib.sf_gather_rows768(x_, ldx, im, y_, dt, ldy, rows, None)   # noqa: E731
    assert ga() == 0
    _refused(lib, ga(ldx=769), 'multiple of 4')
    _refused(lib, ga(ldy=770), 'multiple of 4')
    _refused(lib, ga(ldy=770, y_=YB, dt=1), 'multiple of 4')
    for kw in (dict(x_=X + 4), dict(y_=Y + 8), dict(y_=YB + 4, dt=1)):
        _refused(lib, ga(**kw), 'aligned')
    assert ga(y_=YB + 8, dt=1) == 0
    br = lambda d_=Y, ld=776, t_=X: lib.sf_broadcast_rows768(d_, ld, 4, t_, 2, 0, None)                                          # noqa: E731
    assert br() == 0
    _refused(lib, br(ld=770), 'bad shape')
    _refused(lib, br(d_=Y + 4), 'aligned')
    _refused(lib, br(t_=X + 8), 'aligned')
    asl = lambda br_=X, res_=X, x_=Y, g_=GA, b_=BE, y_=YB, ldy=776: lib.sf_add_scale_ln768(br_, 776, None, 1, res_, 776, x_, 776, g_, b_, y_, ldy, 0, 1e-6, None)   # noqa: E731
    assert asl() == 0
    _refused(lib, asl(ldy=770), 'multiples of 4')
    for kw in (dict(br_=X + 4), dict(res_=X + 8), dict(x_=Y + 4), dict(g_=GA + 8), dict(b_=BE + 4), dict(y_=YB + 4)):
        _refused(lib, asl(**kw), 'aligned')
    lmx = lambda x_=X, g_=GA, b_=BE, q_=Q: lib.sf_layernorm768_mxfp8(x_, 776, g_, b_, q_, 784, SC, 32, 0, 1e-6, None)             # noqa: E731
    assert lmx() == 0
    for kw in (dict(x_=X + 4), dict(g_=GA + 8), dict(b_=BE + 4), dict(q_=Q + 8)):
        _refused(lib, lmx(**kw), 'aligned')
    # every refusal above came from a check this library has: only now the row count, whose launch a library without the check would attempt
    _refused(lib, ln(rows=1 << 31, im=ident), '2^31')
    _refused(lib, ln(rows=1 << 31, om=ident), '2^31')
    _refused(lib, ga(rows=1 << 31, im=ident), '2^31')
    with pytest.raises(AssertionError):
        ops.gather_rows(torch.zeros(4, 772, device=gpu), torch.zeros(4, 768, device=gpu), 0)
    with pytest.raises(AssertionError):
        ops.gather_rows(torch.zeros(4, 768, device=gpu), torch.zeros(4, 772, device=gpu, dtype=BF16), 0)


# =====================================================================================================================================================
# 2. sf_quantize_mxfp8, sf_layernorm768_mxfp8
# =====================================================================================================================================================
def _mx_outputs(gpu, rows, K, ldq, rows_alloc):
    Q = _Out(gpu, rows, K, U8, ld=ldq, off=16 if ldq > K else 0)
    pre = G.canary((K // 128, rows_alloc, 4), U8)
    return Q, pre, pre.to(gpu)


def _mx_verify(what, Q, pre, planes, rows, q_want, sc_want):
    got_q = Q.get()
    torch.cuda.synchronize()
    got_p = planes.cpu()
    written = torch.zeros_like(pre, dtype=torch.bool)
    written[:, :rows] = True
    dmg = G.canary_damage(got_p, pre, written)
    assert dmg is None, f'{what}: scale planes: {dmg}'
    msg = R.bits_mismatch(G.mx_unplane(got_p, rows), sc_want)
    assert msg is None, f'{what}: scale bytes: {msg}'
    msg = R.bits_mismatch(got_q, q_want)
    assert msg is None, f'{what}: e4m3 bytes: {msg}'


@pytest.mark.parametrize('K', (128, 256, 768, 3072))
@pytest.mark.parametrize('rows', (1, 3, 5, 70))
def test_quantize_mxfp8(gpu, blocks, rows, K):
    """Bytes and scale bytes exact on the constructed blocks (rowops_fwd_oracle.mx_blocks: maxima at the 448 boundary and the clamps of the scale byte, e4m3 ties and
    subnormals, bf16 subnormals, +-0, the all-zero blocks; (70, 3072) holds every one of them), contiguous and with ldx > K, ldq > K, planes of lds > 4 rows.
    rows * K / 32 is a multiple of 256 at none of these shapes: the last block's re-read tail runs in every case."""
    from synchformer_amd import ops
    x = R.mx_matrix(blocks, rows, K, start=0 if (rows, K) == (70, 3072) else rows * 131 + K)
    q_want, sc_want = R.mx_quant_int(x)
    for ldx, ldq, rows_alloc in ((K, K, rows), (K + 8, K + 16, rows + 3)):
        Q, pre, planes = _mx_outputs(gpu, rows, K, ldq, rows_alloc)
        ops.quantize_mxfp8(_place(x, ldx, 8 if ldx > K else 0, gpu), Q.view, planes, rows=rows)
        _mx_verify(f'sf_quantize_mxfp8 {rows} x {K} ld {ldx}/{ldq}', Q, pre, planes, rows, q_want, sc_want)
    _record('sf_quantize_mxfp8', 'e4m3 + e8m0', 'blocks', 0.0)


@pytest.mark.parametrize('rows', (1, 5, 9))
def test_layernorm_mxfp8(gpu, ln_params, rows):
    """sf_layernorm768_mxfp8 == sf_layernorm768 (bf16) followed by sf_quantize_mxfp8, byte for byte, with strided x / q and padded planes; the two links of that chain
    are held to float64 and to the integer oracle above, and the chain's bytes to the oracle's quantisation of the bf16 LayerNorm output."""
    from synchformer_amd import ops
    g, b, gd, bd = ln_params
    for family in ('gauss', 'scales', 'spike'):
        x = R.ln_input(family, rows, seed=30 + rows)
        yb = torch.empty(rows, 768, device=gpu, dtype=BF16)
        ops.layernorm(x.to(gpu), gd, bd, yb, 1e-6)
        q_want, sc_want = R.mx_quant_int(yb.cpu())
        for ldx, ldq, rows_alloc in ((768, 768, rows), (776, 784, rows + 3)):
            Q, pre, planes = _mx_outputs(gpu, rows, 768, ldq, rows_alloc)
            ops.layernorm_mxfp8(_place(x, ldx, _off(ldx), gpu), gd, bd, Q.view, planes, 1e-6, rows=rows)
            _mx_verify(f'sf_layernorm768_mxfp8 {family} rows {rows} ld {ldx}/{ldq}', Q, pre, planes, rows, q_want, sc_want)
        Q, pre, planes = _mx_outputs(gpu, rows, 768, 768, rows)
        ops.quantize_mxfp8(yb, Q.view, planes, rows=rows)
        _mx_verify(f'sf_quantize_mxfp8 of the bf16 LayerNorm, {family} rows {rows}', Q, pre, planes, rows, q_want, sc_want)
    _record('sf_layernorm768_mxfp8', 'e4m3 + e8m0', 'gauss, scales, spike', 0.0)


# =====================================================================================================================================================
# 3. sf_broadcast_rows768, sf_gather_rows768
# =====================================================================================================================================================
@pytest.mark.parametrize('n_seq', (1, 3))
@pytest.mark.parametrize('L', (1, 5))
def test_broadcast_rows(gpu, L, n_seq):
    from synchformer_amd import ops
    table = R.f32_probes((L, 768), seed=L)
    for ld in (768, 776):
        seq_rows = L + 2
        idx = (torch.arange(n_seq).unsqueeze(1) * seq_rows + torch.arange(L).unsqueeze(0)).reshape(-1)
        O = _Out(gpu, n_seq * L, 768, F32, ld=ld, off=_off(ld), rows=n_seq * seq_rows + 1, idx=idx)
        ops.broadcast_rows(O.view, table.to(gpu), n_seq=n_seq, dst_seq_rows=seq_rows)
        msg = R.bits_mismatch(O.get(), table.repeat(n_seq, 1))
        assert msg is None, f'L {L} n_seq {n_seq} ld {ld}: {msg}'
    _record('sf_broadcast_rows768', 'fp32', 'bit patterns', 0.0)


@pytest.mark.parametrize('in_map', (None, (1, 1, 3, 0, 0, 0), (4, 4, 5, 0, 1, 1)), ids=('identity', 'cls', 'dropcls'))
def test_gather_rows(gpu, in_map):
    """A bit-exact move (fp32) or one round-to-nearest-even (bf16) of inputs on exact bf16 ties, one fp32 ulp to either side, +-inf and fp32 subnormals."""
    from synchformer_amd import ops
    i = 0
    for rows in ROWS:
        x = R.f32_probes((rows, 768), seed=rows)
        src = R.map_rows(in_map, rows)
        xin = torch.full((int(src.max()) + 2, 768), float('nan'))
        xin[src] = x
        for dtype in (F32, BF16):
            ldx, ldy = LDS[i % 4]
            i += 1
            O = _Out(gpu, rows, 768, dtype, ld=ldy, off=_off(ldy))
            ops.gather_rows(_place(xin, ldx, _off(ldx), gpu), O.view, rows, in_map=in_map)
            msg = R.bits_mismatch(O.get(), x if dtype == F32 else R.rne_bf16_bits(x))
            assert msg is None, f'rows {rows} {dtype} ld {ldx}/{ldy}: {msg}'
    _record('sf_gather_rows768', 'fp32, bf16', 'bit patterns', 0.0)


# =====================================================================================================================================================
# 4. the patch gathers
# =====================================================================================================================================================
VID_DTYPES = (U8, F16, BF16, F32)
_IDS = {U8: 'u8', F16: 'f16', BF16: 'bf16', F32: 'f32'}


@pytest.mark.parametrize('dtype', VID_DTYPES, ids=lambda d: _IDS[d])
def test_im2col_video(gpu, dtype):
    """Two segments: every output element against the value its input element must arrive as (u8: the float16 table; f16 / f32: one RNE; bf16: the same bits)."""
    from synchformer_amd import ops
    vid, want = R.video_input(dtype, (2, 16, 3, 224, 224), seed=41)
    O = _Out(gpu, 2 * 1568, 1536, BF16, rows=2 * 1568 + 2)
    ops.im2col_video(vid.to(gpu), O.buf[:2 * 1568])
    msg = R.bits_mismatch(O.get(), R.video_patches(want))
    assert msg is None, msg
    _record('sf_im2col_video', 'bf16', _IDS[dtype], 0.0)


@pytest.mark.parametrize('dtype', VID_DTYPES, ids=lambda d: _IDS[d])
def test_im2col_video_clips(gpu, dtype):
    """Segments read in place from 2 clips of 23 frames (the element size enters the address: every dtype); a window that does not fit is refused."""
    from synchformer_amd import ops
    vid, want = R.video_input(dtype, (2, 23, 3, 224, 224), seed=42)
    vd = vid.to(gpu)
    for frame0, stride, n_seg in ((3, 4, 2), (7, 0, 1), (0, 7, 2)):
        n = 2 * n_seg
        O = _Out(gpu, n * 1568, 1536, BF16, rows=n * 1568 + 2)
        ops.im2col_video_clips(vd, O.buf, frame0, stride, n_seg)
        msg = R.bits_mismatch(O.get(), R.video_patches(R.clip_segments(want, frame0, stride, n_seg)))
        assert msg is None, f'frame0 {frame0} stride {stride} n_seg {n_seg}: {msg}'
    out = torch.empty(2 * 1568, 1536, device=gpu, dtype=BF16)
    for frame0, stride, n_seg in ((8, 0, 1), (0, 8, 2), (-1, 0, 1)):
        with pytest.raises(RuntimeError, match='do not fit'):
            ops.im2col_video_clips(vd, out, frame0, stride, n_seg)
    _record('sf_im2col_video_clips', 'bf16', _IDS[dtype], 0.0)


@pytest.mark.parametrize('n_seg', (1, 3))
def test_im2col_video_tokens(gpu, n_seg):
    """The token layout: the CLS row of every segment turns from canary to zero (96 runs per segment behind exactly 588 full blocks of patch runs), the patches follow
    at rows 1 .. 1568, rows beyond the last segment keep the canary."""
    from synchformer_amd import ops
    for dtype in (U8, F32):
        vid, want = R.video_input(dtype, (1, 24, 3, 224, 224), seed=43)
        frame0, stride = (1, 3) if n_seg == 3 else (5, 0)
        O = _Out(gpu, n_seg * 1569, 1536, BF16, rows=n_seg * 1569 + 2)
        ops.im2col_video_tokens(vid.to(gpu), O.buf, frame0, stride, n_seg)
        exp = torch.zeros(n_seg, 1569, 1536, dtype=BF16)
        exp[:, 1:] = R.video_patches(R.clip_segments(want, frame0, stride, n_seg)).view(n_seg, 1568, 1536)
        msg = R.bits_mismatch(O.get(), exp.view(-1, 1536))
        assert msg is None, f'{dtype}: {msg}'
    with pytest.raises(RuntimeError, match='do not fit'):
        ops.im2col_video_tokens(vid.to(gpu), O.buf, 9, 0, 1)
    _record('sf_im2col_video_tokens', 'bf16', 'u8, f32', 0.0)


@pytest.mark.parametrize('n_seg', (1, 3))
@pytest.mark.parametrize('shape', SPEC_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_im2col_spec(gpu, shape, n_seg):
    """Conv2d(k 16, stride 10) patches via unfold; (37, 29) and (26, 17) end in rows / columns that no patch covers."""
    from synchformer_amd import ops
    F, Ta = shape
    spec = R.f32_probes((n_seg, F, Ta), seed=F)
    rows = n_seg * ((F - 16) // 10 + 1) * ((Ta - 16) // 10 + 1)
    O = _Out(gpu, rows, 256, BF16, rows=rows + 2)
    ops.im2col_spec(spec.to(gpu), O.buf)
    msg = R.bits_mismatch(O.get(), R.rne_bf16_bits(R.spec_patches(spec)))
    assert msg is None, msg
    _record('sf_im2col_spec', 'bf16', f'{F}x{Ta}', 0.0)


# =====================================================================================================================================================
# 5. token masks
# =====================================================================================================================================================
@pytest.mark.parametrize('n_seg', (1, 2))
def test_token_mask_video(gpu, n_seg):
    """Crafted filter signs (+1, -1, 0) and masks: nothing masked, one masked pixel on a + weight (kept), on a 0 weight (dropped), one + and one - (dropped), two of a sign
    (kept), at runs 0, 63, 64, 95 (the wave's second trip) and pixels 0, 15, in both frames of the pair; the neighbours of every such patch stay kept."""
    from synchformer_amd import ops
    w0s = R.video_w0_sign()
    keep, want = R.video_mask_cases(n_seg)
    lit = R.token_keep_literal(R.video_patches(keep).view(n_seg, 1568, 1536), w0s.double())
    assert torch.equal(lit.to(U8), want[:, 1:])
    pre = G.canary((n_seg * 1569 + 64,), U8)
    out = pre.to(gpu)
    ops.token_mask_video(keep.to(gpu), w0s.to(gpu), out)
    got = out.cpu()
    assert torch.equal(got[n_seg * 1569:], pre[n_seg * 1569:]), 'bytes behind the n * 1569 flags were written'
    bad = (got[:n_seg * 1569].view(n_seg, 1569) != want).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} token flags differ, first (segment, token) {bad[0].tolist()}'
    _record('sf_token_mask_video', 'u8', 'crafted', 0.0)


@pytest.mark.parametrize('n_seg', (1, 2))
@pytest.mark.parametrize('shape', SPEC_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_token_mask_spec(gpu, shape, n_seg):
    from synchformer_amd import ops
    F, Ta = shape
    ws = R.spec_w0_sign()
    keep = R.spec_mask_cases(n_seg, F, Ta, seed=F + n_seg)
    want = R.spec_token_keep(keep, ws)
    L = want.shape[1]
    pre = G.canary((n_seg * L + 64,), U8)
    out = pre.to(gpu)
    ops.token_mask_spec(keep.to(gpu), ws.to(gpu), out)
    got = out.cpu()
    assert torch.equal(got[n_seg * L:], pre[n_seg * L:]), 'bytes behind the flags were written'
    assert (got[:n_seg * L].view(n_seg, L)[:, :2] == 1).all()
    bad = (got[:n_seg * L].view(n_seg, L) != want).nonzero()
    assert bad.numel() == 0, f'{bad.shape[0]} token flags differ, first (segment, token) {bad[0].tolist()}'
    _record('sf_token_mask_spec', 'u8', f'{F}x{Ta}', 0.0)


# =====================================================================================================================================================
# 6. the mel front-end
# =====================================================================================================================================================
class _Mel:
    """The tables of one n_mels on the host and the device, and direct calls of the sf_mel_frontend* entries into a canaried output with spare rows."""

    def __init__(self, gpu, lib, n_mels):
        from synchformer_amd import frontend
        self.gpu, self.lib, self.n_mels = gpu, lib, n_mels
        self.mean, self.std = frontend.AST_MEAN, frontend.AST_STD
        self.host = frontend.mel_tables(n_mels)
        self.dev = {k: torch.from_numpy(v).to(gpu) for k, v in self.host.items()}

    def _tail(self, n_seg, n, pad_to, hop=160):
        frames = min(n // 160 + 1, pad_to)
        self.ws = torch.empty(max(1, n_seg * frames * 513), device=self.gpu)
        O = _Out(self.gpu, n_seg * self.n_mels, pad_to, F32)
        d = self.dev
        return O, (n, hop, d['tw_cos'].data_ptr(), d['tw_sin'].data_ptr(), d['fb'].data_ptr(), d['fb_lo'].data_ptr(), d['fb_hi'].data_ptr(), self.n_mels,
                   self.ws.data_ptr(), O.buf.data_ptr(), pad_to, self.mean, self.std, torch.cuda.current_stream().cuda_stream)

    def run(self, wave, pad_to, hop=160, n=None, check=True):
        """sf_mel_frontend on wave (n_seg, n) (host) -> (n_seg, n_mels, pad_to) on the host, the canary checked; with check=False the return code."""
        n_seg = wave.shape[0]
        n = wave.shape[1] if n is None else n
        O, tail = self._tail(n_seg, n, pad_to, hop)
        wd = wave.to(self.gpu)
        rc = self.lib.sf_mel_frontend(wd.data_ptr(), n_seg, *tail)
        if not check:
            return rc
        assert rc == 0, self.lib.sf_last_error().decode()
        return O.get().view(n_seg, self.n_mels, pad_to)

    def clips(self, wave_d, sample0, stride, n_seg, n, pad_to, check=True):
        """sf_mel_frontend_clips (sample0 an int) or sf_mel_frontend_starts (sample0 a device int64 tensor) on wave_d (n_clips, clip_samples) on the device."""
        B, clip = wave_d.shape
        O, tail = self._tail(B * n_seg, n, pad_to)
        if isinstance(sample0, int):
            rc = self.lib.sf_mel_frontend_clips(wave_d.data_ptr(), B, clip, sample0, stride, n_seg, *tail)
        else:
            rc = self.lib.sf_mel_frontend_starts(wave_d.data_ptr(), B, clip, sample0.data_ptr(), stride, n_seg, *tail)
        if not check:
            return rc
        assert rc == 0, self.lib.sf_last_error().decode()
        return O.get().view(B * n_seg, self.n_mels, pad_to)


@pytest.fixture(scope='module')
def mels(gpu, lib):
    return {n: _Mel(gpu, lib, n) for n in (128, 40)}


# (n_samples, pad_to, n_mels, n_seg): 513 the minimum (4 frames), 5000 (32 frames: a partial group of 13), 10240 (65), 10400 (66 = pad_to), 10560 (67: truncated), 11111 (odd)
MEL_CASES = ((513, 66, 128, 3), (5000, 66, 128, 3), (10240, 66, 128, 1), (10400, 66, 128, 1), (10560, 66, 128, 3), (11111, 66, 128, 1), (5000, 8, 128, 1), (5000, 66, 40, 3),
             (513, 66, 40, 1))


@pytest.mark.parametrize('family', R.MEL_FAMILIES)
def test_mel_frontend(mels, family):
    """Every case of MEL_CASES: the padded frames bit for bit, every element within its bar where the bar holds (everywhere, for the non-tonal families: the bar stays
    below 5e-3 there), and for tones and DC the per-frame l2 criterion against the fp32 emulation."""
    tonal = family in R.MEL_TONAL
    for n, pad_to, n_mels, n_seg in MEL_CASES:
        m = mels[n_mels]
        w = R.mel_wave(family, n_seg, n, seed=n + n_seg)
        got = m.run(w, pad_to)
        exp = R.mel_reference(w, m.host, pad_to, m.mean, m.std)
        emu = R.mel_emulate(w, m.host, pad_to, m.mean, m.std) if tonal else None
        res = R.mel_check(got, exp, emu)
        print(f'sf_mel_frontend {family} n {n} pad_to {pad_to} n_mels {n_mels} n_seg {n_seg}: worst err / bar {res["worst"]:.3g}, bar max {float(exp["bar"].max()):.3g}, '
              f'share under the cap {res["share"]:.3f}, worst frame ratio {res["frame"]:.3g}')
        if not tonal:
            assert float(exp['bar'].max()) < R.MEL_CAP, float(exp['bar'].max())
        assert res['msg'] is None, f'{family} n {n} pad_to {pad_to} n_mels {n_mels} n_seg {n_seg}: {res["msg"]}'
        _record('sf_mel_frontend', 'fp32', family, res['worst'], res['frame'], res['share'])


def test_mel_frontend_clips_and_starts(mels):
    """_clips (an odd sample0, a stride, 2 clips) bit for bit equal to the per-segment call on host-sliced segments; _starts equal to that at per-clip starts, and
    entries below 0 / above max_start equal to their clamped values."""
    m = mels[128]
    n, stride, n_seg, pad_to = 5000, 3001, 2, 66
    clip = 77 + stride + n + 13
    wave = R.mel_wave('noise', 2, clip, seed=5)
    wd = wave.to(m.gpu)
    sliced = lambda starts: torch.stack([wave[c, s0 + s * stride: s0 + s * stride + n] for c, s0 in enumerate(starts) for s in range(n_seg)])   # noqa: E731
    got = m.clips(wd, 77, stride, n_seg, n, pad_to)
    assert R.bits_mismatch(got, m.run(sliced((77, 77)), pad_to)) is None
    st = lambda a, b: torch.tensor([a, b], dtype=torch.int64, device=m.gpu)                                                                      # noqa: E731
    assert R.bits_mismatch(m.clips(wd, st(77, 77), stride, n_seg, n, pad_to), got) is None
    assert R.bits_mismatch(m.clips(wd, st(12, 89), stride, n_seg, n, pad_to), m.run(sliced((12, 89)), pad_to)) is None
    max_start = clip - stride - n
    assert R.bits_mismatch(m.clips(wd, st(-5, 10 ** 9), stride, n_seg, n, pad_to), m.clips(wd, st(0, max_start), stride, n_seg, n, pad_to)) is None
    assert R.bits_mismatch(m.clips(wd, st(0, max_start), stride, n_seg, n, pad_to), m.run(sliced((0, max_start)), pad_to)) is None


def test_mel_frontend_refuses(mels):
    m = mels[128]
    w = torch.zeros(2, 6000)
    _refused(m.lib, m.run(w, 66, hop=161, check=False), 'hop 161 unsupported')
    _refused(m.lib, m.run(w, 66, n=512, check=False), 'shorter than the reflect padding')
    wd = w.to(m.gpu)
    _refused(m.lib, m.clips(wd, 1, 500, 2, 5500, 66, check=False), 'do not fit')
    _refused(m.lib, m.clips(wd, -1, 0, 1, 5000, 66, check=False), 'do not fit')
    _refused(m.lib, m.clips(wd, torch.zeros(2, dtype=torch.int64, device=m.gpu), 600, 2, 5500, 66, check=False), 'do not fit')
