"""GPU: the GEMM family (csrc/sf_gemm.hip, sf_gemm_pp.hip, sf_gemm_w4.hip, sf_gemm_ln.hip, sf_gemm_ln2.hip, sf_gemm_mx.hip, sf_gemm_ln_mx.hip) against float64 at the
k-depths, row strides, epilogues and tile walks the workload's own shapes never reach.  The oracle, the operand families and both acceptance criteria are
tests/gemm_oracle.py (its docstring states the bars; tests/test_gemm_oracle_cpu.py shows that they reject a subtly wrong kernel).

Conventions of every test below (those of tests/test_train_rowops_gpu.py and tests/test_attention_fwd_gpu.py):
  - the float64 reference is computed from the very bf16 / e4m3 values the kernel reads; every written element is compared;
  - family `exact` (integer operands): fp32 outputs equal the int64 result BIT FOR BIT, bf16 outputs equal its single rounding bit for bit, whatever the
    summation order, tiling or k rotation; GELU outputs are held to the `wide` bar around the exact pre-activation;
  - family `wide`: elementwise |got - ref| <= 1.5 (u_out |ref| + (d + c) 2^-24 S) AND per 64 x 64 block ||got - ref|| <= 2 ||emu - ref|| + ||F||;
  - every output buffer is pre-filled with a position-dependent canary (NaNs whose payload is the element index) that must survive bit for bit wherever the
    kernel must not write: rows beyond M, the pad columns of a strided output, unmapped rows, the gaps between batches;
  - A rows beyond M, and the pad columns of every strided operand, are NaN (0x7F bytes / 0xFF scale bytes for MXFP8);
  - strided operands are column slices of wider buffers; every view starts 16-byte aligned and keeps the stride multiples its launcher demands; every launch
    stays inside the launcher's argument checks (a refusal is asserted, never provoked on the device).

d (longest chain of dependent fp32 additions behind one accumulator = MFMA steps along k + the k-extent of one MFMA, gemm_oracle.depth) and c per kernel:
  gemm_bf16_kernel (configs 0 - 6, 8, 9; sf_gemm_bf16_batched)            v_mfma_f32_16x16x32_bf16: d = K / 32 + 32, c = 2 ((acc + bias) + residual)
  persistent / quadrant-phased / 4-wave / r4 kernels (7, 11, 10, 12), dual  v_mfma_f32_32x32x16_bf16: d = K / 16 + 16, c = 2 (a k rotation permutes the chain, not its length)
  sf_gemm_res_ln768(_periodic), schedules 0, 1, 2                          v_mfma_f32_32x32x16_bf16: d = K / 16 + 16, c = 2; Y: the LayerNorm bar of the oracle
  sf_gemm_mxfp8, sf_gemm_mx_res_ln768                                      v_mfma_scale_f32_32x32x64_f8f6f4: d = K / 64 + 64, c = 2, + gemm_oracle.mx_group_term
The MXFP8 bars carry one term ADDED AFTER THE FIRST MEASUREMENT: with d and c alone the `wide` family missed the elementwise bar by up to 14 x (about 2^-15.5 of S)
while the `exact` family was bit-exact at every shape, schedule and epilogue.  The cause is the matrix instruction, not the kernels: probed with one large product
next to smaller ones, v_mfma_scale_f32_32x32x64_f8f6f4 aligns the products of a group of 8 consecutive k to the group's largest and drops what lies below 2^-13 of its
power of two, while sums across groups, 32-blocks and k-steps behave like fp32.  Hence 7 * 2^-13 * sum over 8-groups of max |a_k w_k| on top of (d + c) 2^-24 S; the
bf16 kernels' bars needed nothing.

What the tests cannot see: which tile configuration, schedule or epilogue path a launch really took.  sf_gemm_force_config / the schedule hooks are
trusted, and the launcher chooses between the buffer-op and the general epilogue silently, from N, the row maps and the alignment of pointers and strides;
for the automatic choice d is taken from sf_gemm_bf16_auto_config (0 at every shape here but the tile walks, where a configuration is forced).  A launch that
took another path than intended would still be held to a bar - the bit-exact `exact` family does not depend on d at all, and carries the weight.

Measured on the MI355X over all cases of a kernel (set SF_GEMM_TEST_STATS=<file> to have every check append its figures).  output: linear = no activation,
GELU, Y = the LayerNorm output (elementwise bar only), with the output type.  The `exact` family has figures for GELU and Y only: everything else in it is compared bit for bit.
  kernel                        output       family  checks  worst err / bar  worst block ||got - ref|| / limit
  sf_gemm_bf16                  GELU bf16    exact       25            0.664       0.500
  sf_gemm_bf16                  GELU bf16    wide        25            0.663       0.499
  sf_gemm_bf16                  GELU fp32    exact       35            0.606       0.036
  sf_gemm_bf16                  GELU fp32    wide        35            0.367       0.012
  sf_gemm_bf16                  linear bf16  wide       199            0.664       0.499
  sf_gemm_bf16                  linear fp32  wide       229            0.130       0.021
  sf_gemm_bf16_batched          linear bf16  wide        60            0.663       0.499
  sf_gemm_bf16_batched          linear fp32  wide        60            0.072       0.014
  sf_gemm_bf16_gelu_dual        GELU bf16    exact        2            0.664       0.500
  sf_gemm_bf16_gelu_dual        GELU bf16    wide         2            0.660       0.499
  sf_gemm_bf16_gelu_dual        linear bf16  wide         2            0.662       0.499
  sf_gemm_mx_res_ln768          Y bf16       exact       12            0.955           -
  sf_gemm_mx_res_ln768          Y bf16       wide        12            0.937           -
  sf_gemm_mx_res_ln768          linear fp32  wide        12            0.283       0.103
  sf_gemm_mxfp8                 GELU bf16    exact      108            0.664       0.500
  sf_gemm_mxfp8                 GELU bf16    wide       108            0.656       0.373
  sf_gemm_mxfp8                 GELU fp32    exact      108            0.634       0.070
  sf_gemm_mxfp8                 GELU fp32    wide       108            0.245       0.055
  sf_gemm_mxfp8                 linear bf16  wide       162            0.629       0.395
  sf_gemm_mxfp8                 linear fp32  wide       162            0.276       0.067
  sf_gemm_res_ln768             Y bf16       exact      121            0.500           -
  sf_gemm_res_ln768             Y bf16       wide       121            0.499           -
  sf_gemm_res_ln768             linear fp32  wide       121            0.168       0.025
  sf_gemm_res_ln768_periodic    Y bf16       exact        8            0.500           -
  sf_gemm_res_ln768_periodic    Y bf16       wide         8            0.499           -
  sf_gemm_res_ln768_periodic    linear fp32  wide         8            0.124       0.016
A bf16 output's 0.66 / 0.50 are the rounding itself (half an ulp is at most 2 / 3 of 1.5 * 2^-8 |ref|; the emulation rounds the same way), so the fp32 rows are
the ones that measure the kernels: the bf16-operand kernels use 0.07 - 0.17 of the worst-case chain bound (d + c) 2^-24 S written before the first run, the
MXFP8 kernels 0.28 of a bar that mx_group_term dominates - the instruction's truncation reaches 0.4 of its worst case, the term is no order of magnitude slack
(tests/test_gemm_oracle_cpu.py states what it can no longer reject).  The MXFP8 Y at 0.95 is the e4m3 step of an element next to its block's saturation."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ('exact', 'wide')
PRODUCT_CFGS = (-1, 0, 4, 7, 11)
ABLATION_CFGS = (1, 2, 3, 5, 6, 8, 9, 10, 12)
MFMA = {c: '16x16x32' for c in (0, 1, 2, 3, 4, 5, 6, 8, 9)}
MFMA.update({c: '32x32x16' for c in (7, 10, 11, 12)})
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
_STATS_PATH = os.environ.get('SF_GEMM_TEST_STATS')


# =====================================================================================================================================================
# plumbing
# =====================================================================================================================================================
def _place(t, ld, off, dev, rows=None):
    """t (r, c) as the column slice [off, off + c) of a (rows >= r, ld) buffer whose every other element is NaN (0x7F for bytes); returns the device view."""
    r, c = t.shape
    rows = r if rows is None else rows
    if ld == c and off == 0 and rows == r:
        return t.to(dev)
    assert off + c <= ld and rows >= r
    buf = torch.full((rows, ld), 0x7F, dtype=U8) if t.dtype == U8 else torch.full((rows, ld), float('nan'), dtype=t.dtype)
    buf[:r, off:off + c] = t
    return buf.to(dev)[:, off:off + c]


class _Out:
    """An output buffer (rows, ld) filled with the position-dependent canary; the kernel may write the N columns from `off` of the physical rows `idx`
    (default: rows 0 .. M - 1).  init: what those elements hold before the launch (an in-place residual).  get() checks the canary bit for bit and returns
    the written (len(idx), N) block, on the host - or on the device with on_device, for the outputs too large to bring back in a quick test."""

    def __init__(self, dev, M, N, dtype, ld=None, off=0, rows=None, idx=None, init=None, on_device=False):
        ld = N if ld is None else ld
        rows = M + 3 if rows is None else rows
        where = dev if on_device else 'cpu'
        self.idx = (torch.arange(M) if idx is None else idx).to(where)
        self.off, self.N = off, N
        self.pre = G.canary((rows, ld), dtype).to(where)
        self.written = torch.zeros((rows, ld), dtype=torch.bool, device=where)
        self.written[self.idx, off:off + N] = True
        if init is not None:
            self.pre[self.idx, off:off + N] = init.to(where)
        self.buf = self.pre.to(dev).clone() if on_device else self.pre.to(dev)
        self.view = self.buf[:, off:off + N]
        self.where = where

    def get(self):
        torch.cuda.synchronize()
        got = self.buf.to(self.where)
        dmg = G.canary_damage(got, self.pre, self.written)
        assert dmg is None, dmg
        return got[self.idx, self.off:self.off + self.N]


def _record(kernel, what, elem, stat):
    if _STATS_PATH:
        with open(_STATS_PATH, 'a') as f:
            f.write(f'{kernel}\t{what}\t{elem:.4g}\t{stat:.4g}\n')


def _verify(kernel, what, family, got, exp, emu, out_bf16, gelu=False):
    """The family's acceptance of one output block `got` (host or device, like exp / emu)."""
    if family == 'exact' and not gelu:
        msg = G.exact_mismatch(got, exp['ref'], out_bf16)
        assert msg is None, f'{kernel} {what}: {msg}'
        return
    r = G.wide_check(got.float(), exp, emu)
    _record(kernel, f'{family} {what}', r['elem'], r['stat'])
    assert r['msg'] is None, f'{kernel} {what}: {r["msg"]}'


_op_cache, _pre_cache = {}, {}


def _ops(family, M, N, K, dev=None):
    key = (family, M, N, K, str(dev))
    if key not in _op_cache:
        if len(_op_cache) > 6:
            _op_cache.clear()
            _pre_cache.clear()
        op = G.operands(family, M, N, K, seed=(M * 131 + N) * 7 + K + (family == 'wide'))
        if dev is not None:
            op = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in op.items()}
        _op_cache[key] = op
    return _op_cache[key]


def _pre(family, M, N, K, bias, dev=None):
    key = (family, M, N, K, bias, str(dev))
    if key not in _pre_cache:
        op = _ops(family, M, N, K, dev)
        _pre_cache[key] = G.reference(op['a'][:M], op['w'], op['bias'] if bias else None)
    return _pre_cache[key]


def _expect(family, M, N, K, *, bias, res, gelu, out_bf16, mfma, dev=None):
    """(exp, emu) of out = act(a w^T + bias) (+ res) for the cached operands of (family, M, N, K)."""
    op = _ops(family, M, N, K, dev)
    pre, S = _pre(family, M, N, K, bias, dev)
    r = op['res'] if res else None
    exp = G.expected(pre, S, r, gelu=gelu, out_bf16=out_bf16, d=G.depth(K, mfma), exact_pre=family == 'exact')
    emu = None
    if family == 'wide' or gelu:
        emu = G.emulate(op['a'][:M], op['w'], op['bias'] if bias else None, r, gelu=gelu, out_bf16=out_bf16)
    return exp, emu


@contextlib.contextmanager
def _forced(cfg):
    """sf_gemm_bf16 launches inside run tile configuration `cfg` - in the product library, or in the ablation build for the configurations only it carries."""
    from synchformer_amd import _lib
    lib = _lib.load() if cfg in PRODUCT_CFGS else _lib.load_ablation()
    with _lib.using(lib):
        lib.sf_gemm_force_config(cfg)
        try:
            yield lib
        finally:
            lib.sf_gemm_force_config(-1)


def _mfma_of(cfg, M, N, K, res):
    if cfg >= 0:
        return MFMA[cfg]
    from synchformer_amd import _lib
    return MFMA[_lib.load().sf_gemm_bf16_auto_config(M, N, K, int(bool(res)))]


def _gemm_once(dev, family, M, N, K, cfg, *, out_bf16, gelu=False, res=None, bias=True, lda=None, ldw=None, ldc=None, ldr=None, off=0, on_device=False, what=''):
    """One sf_gemm_bf16 launch on the cached operands and its verification.  res: None, 'inplace' (fp32 output only: R is C) or 'separate'."""
    from synchformer_amd import ops
    op = _ops(family, M, N, K, dev if on_device else None)
    a = _place(op['a'], lda or K, off, dev)
    w = _place(op['w'], ldw or K, off, dev)
    out = _Out(dev, M, N, BF16 if out_bf16 else F32, ld=ldc, off=off, init=op['res'] if res == 'inplace' else None, on_device=on_device)
    r = out.view if res == 'inplace' else (_place(op['res'], ldr or N, off, dev, rows=M + 3) if res == 'separate' else None)
    ops.gemm(a, w, op['bias'].to(dev) if bias else None, out.view, M=M, residual=r, gelu=gelu)
    got = out.get()
    exp, emu = _expect(family, M, N, K, bias=bias, res=res is not None, gelu=gelu, out_bf16=out_bf16, mfma=_mfma_of(cfg, M, N, K, res),
                       dev=dev if on_device else None)
    _verify('sf_gemm_bf16', f'cfg {cfg} {M}x{N}x{K} {"bf16" if out_bf16 else "f32"} gelu={int(gelu)} res={res} bias={int(bias)} {what}', family, got, exp, emu,
            out_bf16, gelu)


# =====================================================================================================================================================
# 1. sf_gemm_bf16
# =====================================================================================================================================================
K_DEPTHS = (64, 128, 192, 256, 320, 384, 448, 512, 640)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', PRODUCT_CFGS, ids=lambda c: 'auto' if c < 0 else f'cfg{c}')
def test_gemm_bf16_k_depth(gpu, cfg, family):
    """k-depths around the ring depths at M = 300, N = 192 (a multiple of 64 but not of 128: one wave tile of the last column tile stores nothing): config 0
    (BK 64, 2 slots) runs nk = 1 .. 10, odd counts included; config 4 (BK 32, 4 slots) nk = 2 (a prologue shorter than the ring), 4, ...; the persistent
    kernel nk = 1 (`if (nk > 1) stage(1, 1)`) and 2; config 11 its minimum of two k-tile pairs - and refuses what its check does not admit."""
    from synchformer_amd import ops
    M, N = 300, 192
    with _forced(cfg):
        for K in K_DEPTHS:
            if cfg == 11 and (K % 128 or K < 256):
                z = torch.zeros(M, K, device=gpu, dtype=BF16)
                with pytest.raises(RuntimeError, match='config 11 needs'):
                    ops.gemm(z, torch.zeros(N, K, device=gpu, dtype=BF16), None, torch.empty(M, N, device=gpu))
                continue
            for out_bf16 in (False, True):
                _gemm_once(gpu, family, M, N, K, cfg, out_bf16=out_bf16)


def _ablation_admits(cfg, K, out_bf16):
    """sf_gemm_bf16's own check for the configurations of the ablation build at (300, 192 | 256, K), contiguous operands, bias, no residual: config 12 serves a
    bf16 output with N % 128 == 0, K % 128 == 0, K >= 256 (sf_gemm_r4_supported); the others every K % 64 == 0."""
    return cfg != 12 or (out_bf16 and K % 128 == 0 and K >= 256)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', ABLATION_CFGS, ids=lambda c: f'cfg{c}')
def test_gemm_bf16_k_depth_ablation_configs(gpu, cfg, family):
    """The same k-depth list on the ablation library's configurations (N = 256 for config 12, whose check demands N % 128 == 0); a shape a configuration's
    check refuses is asserted to be refused."""
    from synchformer_amd import ops
    M, N = 300, (256 if cfg == 12 else 192)
    with _forced(cfg):
        for K in K_DEPTHS:
            for out_bf16 in (False, True):
                if not _ablation_admits(cfg, K, out_bf16):
                    with pytest.raises(RuntimeError, match='config 12 needs'):
                        ops.gemm(torch.zeros(M, K, device=gpu, dtype=BF16), torch.zeros(N, K, device=gpu, dtype=BF16), None,
                                 torch.empty(M, N, device=gpu, dtype=BF16 if out_bf16 else F32))
                    continue
                _gemm_once(gpu, family, M, N, K, cfg, out_bf16=out_bf16)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', PRODUCT_CFGS, ids=lambda c: 'auto' if c < 0 else f'cfg{c}')
def test_gemm_bf16_epilogue_matrix(gpu, cfg, family):
    """All eight {fp32, bf16} x {GELU} x {residual} instantiations of the fast epilogue, with and without bias, at (257, 320, 256): 3 x 3 = 9 tiles of 128 (not
    a multiple of 8: the XCD remap's remainder branch), 2 x 2 of 256 with a ragged last panel and a 64-column last tile.  The fp32 residual once in place
    and once in a buffer of its own with ldr = N + 12 != ldc; the bf16 output's residual in its own buffer."""
    M, N, K = 257, 320, 256
    with _forced(cfg):
        for out_bf16 in (False, True):
            for gelu in (False, True):
                for res in ((None, 'separate') if out_bf16 else (None, 'inplace', 'separate')):
                    for bias in (True, False):
                        _gemm_once(gpu, family, M, N, K, cfg, out_bf16=out_bf16, gelu=gelu, res=res, bias=bias, ldr=N + 12 if res == 'separate' else None)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', PRODUCT_CFGS, ids=lambda c: 'auto' if c < 0 else f'cfg{c}')
def test_gemm_bf16_row_strides(gpu, cfg, family):
    """A, W, C and R as column slices (from element 8) of wider buffers: lda = K + 64, ldw = K + 8, ldc = N + 8, ldr = N + 12 - the buffer-resource ranges
    M * ldc * esz, the 32-bit coff0 / cstep offsets and the per-lane DMA source offsets ar * lda + chunk * 8 with ld != width.  Pad columns keep their canary."""
    M, N, K = 257, 320, 256
    with _forced(cfg):
        for out_bf16 in (False, True):
            for gelu, res in ((False, 'separate'), (True, None)):
                _gemm_once(gpu, family, M, N, K, cfg, out_bf16=out_bf16, gelu=gelu, res=res, lda=K + 64, ldw=K + 8, ldc=N + 8, ldr=N + 12, off=8, what='strided')


GENERAL_N = ((1, 1), (3, 3), (21, 21), (63, 63), (65, 65), (68, 68), (68, 72), (130, 130))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', (-1, 0, 4), ids=lambda c: 'auto' if c < 0 else f'cfg{c}')
def test_gemm_bf16_general_epilogue(gpu, cfg, family):
    """The general epilogue (N % 64 != 0) at M = 150 (two row tiles, the second ragged), K = 128: N = 1, 3, 21, 63, 65 (scalar stores, the tail `gcol + e < N`),
    68 and 130 (the `vec` branch, N % 4 == 0 without N % 64 == 0, with ldc = N and ldc = 72), fp32 and bf16 output, with and without a residual.  GELU on this
    path is refused, as the dispatcher says."""
    from synchformer_amd import ops
    M, K = 150, 128
    with _forced(cfg):
        for N, ldc in GENERAL_N:
            for out_bf16 in (False, True):
                for res in (None, 'separate') + (() if out_bf16 else ('inplace',)):
                    _gemm_once(gpu, family, M, N, K, cfg, out_bf16=out_bf16, res=res, ldc=ldc, ldr=ldc, bias=N != 65, what=f'ldc={ldc}')
        with pytest.raises(RuntimeError, match='GELU epilogue needs identity row maps'):
            ops.gemm(torch.zeros(M, K, device=gpu, dtype=BF16), torch.zeros(21, K, device=gpu, dtype=BF16), None, torch.empty(M, 21, device=gpu), gelu=True)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('cfg', (-1, 0, 4), ids=lambda c: 'auto' if c < 0 else f'cfg{c}')
def test_gemm_bf16_row_maps(gpu, cfg, family):
    """c_map != r_map: the 200 output rows are four 50-row sequences dropped at row 1 of 51-row sequences of a taller buffer (every 51st row stays canary),
    the residual rows come from a (4 x 25)-transposed layout with another sequence stride; N = 68 (vec branch) and 21 (scalar), fp32 and bf16 output.  The
    reference goes through the row-map formula stated in tests/test_train_rowops_gpu.py::_map_rows."""
    from synchformer_amd import ops

    def map_rows(m, r):
        n12, n2, sA, s1, s2, off = m
        return (r // n12) * sA + ((r % n12) // n2) * s1 + (r % n2) * s2 + off
    M, K = 200, 128
    c_map, r_map = ops.rowmap(50, 50, 51, 0, 1, 1), ops.rowmap(100, 4, 130, 1, 25, 3)
    rows = torch.arange(M)
    c_rows, r_rows = map_rows(c_map, rows), map_rows(r_map, rows)
    assert c_rows.unique().numel() == M and r_rows.unique().numel() == M
    with _forced(cfg):
        for N in (68, 21):
            op = _ops(family, M, N, K)
            a, w, b = op['a'].to(gpu), op['w'].to(gpu), op['bias'].to(gpu)
            rbuf = torch.full((int(r_rows.max()) + 2, N), float('nan'))
            rbuf[r_rows] = op['res']
            rdev = rbuf.to(gpu)
            for out_bf16 in (False, True):
                out = _Out(gpu, M, N, BF16 if out_bf16 else F32, rows=int(c_rows.max()) + 3, idx=c_rows)
                ops.gemm(a, w, b, out.view, M=M, residual=rdev, c_map=c_map, r_map=r_map)
                exp, emu = _expect(family, M, N, K, bias=True, res=True, gelu=False, out_bf16=out_bf16, mfma=_mfma_of(cfg, M, N, K, True))
                _verify('sf_gemm_bf16', f'cfg {cfg} mapped N={N} {"bf16" if out_bf16 else "f32"}', family, out.get(), exp, emu, out_bf16)


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('M,N,K', [(9 * 256 + 1, 1280, 256), (57 * 256 - 100, 1280, 1024)], ids=['10panels', '57panels-chunked'])
@pytest.mark.parametrize('cfg', (7, 11), ids=lambda c: f'cfg{c}')
def test_gemm_bf16_persistent_tile_walk(gpu, cfg, M, N, K, family):
    """The tile walk of the persistent kernels (sf_gemm.hip gemm_bf16_persistent_kernel and sf_gemm_pp.hip share the partition: XCD x owns the row panels
    [x * ceil(tiles_m / 8), ...), gridDim.x / 8 workgroups walk them in column chunks of nchunk = 2400000 / (512 K) tiles when K <= 1024).
    (2305, 1280, 256): 10 panels -> XCD ranges 2, 2, 2, 2, 2, 0, 0, 0 (three XCDs return at once), 56 workgroups = 7 per XCD on 10 tiles: every XCD's workgroups
    0 - 2 walk two tiles, the last of them ragged.  (14492, 1280, 1024): nchunk = 4 -> chunks of 4 + 1 column tiles, 8 panels on seven XCDs and 1 on the last,
    40 tiles per XCD against 32 workgroups, a ragged last panel.  fp32 output with the in-place residual and bf16 output; the float64 reference is a
    torch.matmul in float64 on the device (rocBLAS: independent of the kernels under test), and so is everything derived from it."""
    with _forced(cfg):
        _gemm_once(gpu, family, M, N, K, cfg, out_bf16=False, res='inplace', on_device=True, what='tile walk')
        _gemm_once(gpu, family, M, N, K, cfg, out_bf16=True, on_device=True, what='tile walk')


# =====================================================================================================================================================
# 2. sf_gemm_bf16_batched (through the C ABI, as synchformer_amd.train.bgemm calls it)
# =====================================================================================================================================================
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('M,N,K,b_outer,b_inner', [(198, 198, 96, 2, 3), (5, 7, 32, 2, 3), (130, 128, 512, 3, 2), (130, 192, 576, 3, 2), (130, 100, 512, 3, 2)],
                         ids=['cfg4-198', 'cfg4-5x7', 'cfg0-fast-128', 'cfg0-fast-192', 'cfg0-general-100'])
def test_gemm_bf16_batched(gpu, M, N, K, b_outer, b_inner, family):
    """Cfg4 general path (K < 512), Cfg0 fast path (K % 64 == 0, K >= 512, N % 64 == 0: the batch offset folded into the buffer base) and Cfg0 with the general
    epilogue (N = 100: its vec branch), fp32 and bf16 output, with and without bias.  A and W are packed the way q, k, v sit in a (rows, 2304) buffer: the inner
    batch is a column block (sA1 = sW1 = K < a row), the outer batch a block of rows; C batches sit sC1 > M * ldc and sC0 > b_inner * sC1 apart in one flat
    buffer whose gaps, pad columns and tail keep their canary."""
    from synchformer_amd import _lib
    lib = _lib.load()
    nb = b_outer * b_inner
    ops_ = [G.operands(family, M, N, K, seed=977 * M + 31 * N + K + 5 * i + (family == 'wide'), a_rows=M) for i in range(nb)]
    lda, ldw = b_inner * K + 8, b_inner * K + 16
    abuf = torch.full((b_outer * (M + 1), lda), float('nan'), dtype=BF16)
    wbuf = torch.full((b_outer * (N + 2), ldw), float('nan'), dtype=BF16)
    for i, op in enumerate(ops_):
        b0, b1 = divmod(i, b_inner)
        abuf[b0 * (M + 1):b0 * (M + 1) + M, b1 * K:(b1 + 1) * K] = op['a']
        wbuf[b0 * (N + 2):b0 * (N + 2) + N, b1 * K:(b1 + 1) * K] = op['w']
    ad, wd = abuf.to(gpu), wbuf.to(gpu)
    bias = ops_[0]['bias']
    bd = bias.to(gpu)
    ldc = N + 8 if N % 4 == 0 else N + 5
    sC1 = -(-(M * ldc) // 8) * 8 + 24
    sC0 = b_inner * sC1 + 40
    total = b_outer * sC0 + 64
    base = (torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]).flatten()
    for out_bf16 in (False, True):
        for use_bias in (False, True):
            dtype = BF16 if out_bf16 else F32
            pre = G.canary((total,), dtype)
            written = torch.zeros(total, dtype=torch.bool)
            for i in range(nb):
                b0, b1 = divmod(i, b_inner)
                written[b0 * sC0 + b1 * sC1 + base] = True
            cd = pre.to(gpu)
            rc = lib.sf_gemm_bf16_batched(ad.data_ptr(), lda, (M + 1) * lda, K, wd.data_ptr(), ldw, (N + 2) * ldw, K, bd.data_ptr() if use_bias else None,
                                          cd.data_ptr(), 1 if out_bf16 else 0, ldc, sC0, sC1, M, N, K, b_outer, b_inner, torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, 'sf_gemm_bf16_batched')
            torch.cuda.synchronize()
            got = cd.cpu()
            dmg = G.canary_damage(got, pre, written)
            assert dmg is None, dmg
            for i, op in enumerate(ops_):
                b0, b1 = divmod(i, b_inner)
                g = got[b0 * sC0 + b1 * sC1 + base].view(M, N)
                b = bias if use_bias else None
                p, S = G.reference(op['a'], op['w'], b)
                exp = G.expected(p, S, None, gelu=False, out_bf16=out_bf16, d=G.depth(K, '16x16x32'), exact_pre=family == 'exact')
                emu = G.emulate(op['a'], op['w'], b, None, gelu=False, out_bf16=out_bf16) if family == 'wide' else None
                _verify('sf_gemm_bf16_batched', f'{M}x{N}x{K} batch ({b0}, {b1}) {"bf16" if out_bf16 else "f32"} bias={int(use_bias)}', family, g, exp, emu, out_bf16)


# =====================================================================================================================================================
# 3. sf_gemm_bf16_gelu_dual
# =====================================================================================================================================================
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('M,N,K', [(257, 320, 384), (256, 256, 256)])
def test_gemm_bf16_gelu_dual(gpu, M, N, K, family):
    """pre = bf16(A W^T + bias) and act = bf16(gelu(A W^T + bias)) (the activation of the fp32 pre-activation, sf_gemm_pp.hip) in one launch, both strided
    (ldc = N + 8, column slices from element 8 of two buffers): pre bit-exact in the `exact` family, act within the GELU bar."""
    from synchformer_amd import _lib
    lib = _lib.load()
    op = _ops(family, M, N, K)
    a, w, b = _place(op['a'], K + 64, 8, gpu), _place(op['w'], K + 8, 8, gpu), op['bias'].to(gpu)
    pre, act = _Out(gpu, M, N, BF16, ld=N + 8, off=8), _Out(gpu, M, N, BF16, ld=N + 8, off=8)
    rc = lib.sf_gemm_bf16_gelu_dual(a.data_ptr(), K + 64, w.data_ptr(), K + 8, b.data_ptr(), pre.view.data_ptr(), act.view.data_ptr(), N + 8, M, N, K,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'sf_gemm_bf16_gelu_dual')
    for name, out, gelu in (('pre', pre, False), ('act', act, True)):
        exp, emu = _expect(family, M, N, K, bias=True, res=False, gelu=gelu, out_bf16=True, mfma='32x32x16')
        _verify('sf_gemm_bf16_gelu_dual', f'{M}x{N}x{K} {name}', family, out.get(), exp, emu, True, gelu)


def test_gemm_bf16_gelu_dual_not_applicable(gpu):
    """Outside config 11's range (M = 255 < 256, N = 192 < 256, K = 192) the call returns SF_NOT_APPLICABLE and touches neither buffer."""
    from synchformer_amd import _lib
    lib = _lib.load()
    M, N, K = 255, 192, 192
    a, w = torch.zeros(M, K, device=gpu, dtype=BF16), torch.zeros(N, K, device=gpu, dtype=BF16)
    pre, act = _Out(gpu, 0, N, BF16, rows=M), _Out(gpu, 0, N, BF16, rows=M)
    rc = lib.sf_gemm_bf16_gelu_dual(a.data_ptr(), K, w.data_ptr(), K, None, pre.view.data_ptr(), act.view.data_ptr(), N, M, N, K,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    pre.get()
    act.get()


# =====================================================================================================================================================
# 4. sf_gemm_res_ln768 / sf_gemm_res_ln768_periodic
# =====================================================================================================================================================
D = 768


def _ln_params(seed):
    g = G.gen(seed)
    return 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)


@contextlib.contextmanager
def _res_ln_sched(sched):
    """Schedule 0 / 1 in the product library, schedule 2 in the ablation build."""
    from synchformer_amd import _lib
    lib = _lib.load_ablation() if sched == 2 else _lib.load()
    with _lib.using(lib):
        lib.sf_gemm_res_ln_force_schedule(sched)
        try:
            yield
        finally:
            lib.sf_gemm_res_ln_force_schedule(-1)


def _res_ln_once(dev, family, M, K, *, kmajor, eps=1e-6, lda=None, ldr=None, ldx=None, ldy=None, strided=False, period=None, op=None, on_device=False, what='',
                 mfma='32x32x16', kernel='sf_gemm_res_ln768'):
    """One sf_gemm_res_ln768(_periodic) launch and its verification: X (fp32) as a GEMM output with c = 2, Y (bf16) within the LayerNorm bar around the float64
    LayerNorm of the float64 X, the row's X bar carried through.  X aliases R unless strided / periodic (then R is a buffer of its own).  Returns (x, y) got."""
    from synchformer_amd import ops
    where = dev if on_device else None
    op = _ops(family, M, D, K, where) if op is None else op
    gamma, beta = _ln_params(K + M)
    a = _place(op['a'], lda or K, 8 if strided else 0, dev)
    w = op['w'].to(dev)
    if kmajor:
        w = ops.kmajor_weight(w)
    res = op['res']                                                 # (M, 768), or (period, 768) for the periodic form
    separate = strided or period is not None
    x = _Out(dev, M, D, F32, ld=ldx, off=8 if strided else 0, init=None if separate else res, on_device=on_device)
    y = _Out(dev, M, D, BF16, ld=ldy, off=16 if strided else 0, on_device=on_device)
    r = _place(res, ldr or D, 4 if strided else 0, dev, rows=res.shape[0] + 1) if separate else None
    ops.gemm_res_ln(a, w, op['bias'].to(dev), x.view, gamma.to(dev), beta.to(dev), y.view, eps, M=M, residual=r, period=period)
    xg, yg = x.get(), y.get()
    pre, S = G.reference(op['a'][:M], op['w'], op['bias'])
    rfull = res[torch.arange(M, device=res.device) % period] if period is not None else res
    exp = G.expected(pre, S, rfull, gelu=False, out_bf16=False, d=G.depth(K, mfma), exact_pre=family == 'exact')
    emu = G.emulate(op['a'][:M], op['w'], op['bias'], rfull, gelu=False, out_bf16=False) if family == 'wide' else None
    _verify(kernel, f'X {M}x{K} {what}', family, xg, exp, emu, False)
    ex = exp['bar']                                                 # (>= 2^-24 |X| in the `wide` family: S >= |X|; 0 in the `exact` one, whose X is exact)
    yref, ybar = G.layernorm64(exp['ref'], gamma.to(exp['ref'].device), beta.to(exp['ref'].device), eps, ex)
    err = (yg.double() - yref).abs()
    worst = float((err / ybar).max())
    _record(kernel, f'{family} Y {M}x{K} {what}', worst, 0.0)
    bad = ~(err <= ybar)
    assert not bad.any(), (f'{kernel} Y {M}x{K} {what}: {int(bad.sum())} elements outside the LayerNorm bar (worst err / bar {worst:.3g}), first at '
                           f'{bad.nonzero()[0].tolist()}')
    return xg, yg


RL_K = (32, 64, 96, 128, 192, 256, 320)


def _sched2_admits(K, lda):
    return K % 128 == 0 and lda % 64 == 0


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('sched', (0, 1, 2))
def test_gemm_res_ln_k_depth(gpu, sched, family):
    """K = 32 .. 320 at M = 1, 127, 129 for both weight layouts: nk = 1 (`if (nk > 1) stage(1, 1)`), the quadrant-phased kernel's minimum K = 128 (nk = 4),
    K % 64 != 0 (schedule 1 falls back to round 2's loop), odd nk.  Schedule 2 (ablation build, row-major weight) where its check admits the case: K % 128 == 0."""
    with _res_ln_sched(sched):
        for K in RL_K:
            if sched == 2 and not _sched2_admits(K, K):
                continue                                            # (the launcher then runs schedule 1: covered by that parameter)
            for M in (1, 127, 129):
                for kmajor in ((False,) if sched == 2 else (False, True)):
                    _res_ln_once(gpu, family, M, K, kmajor=kmajor, what=f'sched {sched} kmajor={int(kmajor)}')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('sched', (0, 1, 2))
def test_gemm_res_ln_k_rotation(gpu, sched, family):
    """M = 128 * 48 + 5: workgroups 0 .. 48 give blockIdx.x >> 3 = 0 .. 6, every residue of krot = (blockIdx.x >> 3) % nk for nk <= 6 (K = 64, 128, 192) and
    the wrap of the running offsets (`++kq2 == nk`).  A rotated k-loop sums the same products: the `exact` family stays bit-exact."""
    M = 128 * 48 + 5
    with _res_ln_sched(sched):
        for K in (64, 128, 192):
            if sched == 2 and not _sched2_admits(K, K):
                continue
            for kmajor in ((False,) if sched == 2 else (False, True)):
                _res_ln_once(gpu, family, M, K, kmajor=kmajor, what=f'krot sched {sched} kmajor={int(kmajor)}')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('sched', (0, 1))
def test_gemm_res_ln_tile_loop(gpu, sched, family):
    """M = 128 (n_cu + 1) + 1 at K = 64: n_cu + 2 row tiles on n_cu persistent workgroups - workgroups 0 and 1 take a second tile, its first stages
    prefetched behind the first tile's epilogue, the very last tile holding one row.  Checked on the device."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    with _res_ln_sched(sched):
        _res_ln_once(gpu, family, 128 * (n_cu + 1) + 1, 64, kmajor=True, on_device=True, what=f'tile loop sched {sched}')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('sched', (0, 1, 2))
@pytest.mark.parametrize('M,K', [(129, 128), (300, 768)])
def test_gemm_res_ln_row_strides(gpu, M, K, sched, family):
    """lda = K + 64 and ldr / ldx / ldy = 772 / 776 / 784, every operand a column slice (A from element 8, R 4, X 8, Y 16), R a buffer of its own."""
    with _res_ln_sched(sched):
        for kmajor in ((False,) if sched == 2 else (False, True)):
            _res_ln_once(gpu, family, M, K, kmajor=kmajor, lda=K + 64, ldr=772, ldx=776, ldy=784, strided=True, what=f'strided sched {sched} kmajor={int(kmajor)}')


@pytest.mark.parametrize('eps', [1e-12, 1e-6, 1e-5])
@pytest.mark.parametrize('sched', (0, 1))
def test_gemm_res_ln_normalisation_rows(gpu, sched, eps):
    """Rows that are hard for the normalisation.  (a) `exact` family, A rows 3, 64, 129 zero and bias + residual constant along the row (7 + c, c = -3, 1000, 0):
    X is constant, its centred second moment exactly 0, so Y must equal bf16(beta) BIT FOR BIT whatever eps is (a one-pass variance, or a mean that is not
    the row's value, would give rstd = eps^-1/2 something to amplify).  (b) `wide` family, rows with a common offset of 1000 and unit spread (A row zero,
    residual 1000 + N(0, 1)): the bar carries 2^-24 |mean| / std through the row's X bar and the mean's own rounding; a one-pass variance misses it by orders."""
    M, K = 130, 128
    gamma, beta = _ln_params(K + M)
    const_rows = {3: -3.0, 64: 1000.0, 129: 0.0}
    with _res_ln_sched(sched):
        op = dict(G.operands('exact', M, D, K, seed=5))
        op['a'], op['res'], op['bias'] = op['a'].clone(), op['res'].clone(), torch.full((D,), 7.0)
        for r, c in const_rows.items():
            op['a'][r] = 0
            op['res'][r] = c
        _, yg = _res_ln_once(gpu, 'exact', M, K, kmajor=True, eps=eps, op=op, what=f'constant rows eps {eps:g} sched {sched}')
        for r in const_rows:
            assert torch.equal(G.bits(yg[r]), G.bits(beta.bfloat16())), f'row {r}: a constant row must normalise to beta'
        op = dict(G.operands('wide', M, D, K, seed=6))
        op['a'], op['res'] = op['a'].clone(), op['res'].clone()
        rows = torch.tensor([0, 17, 63, 64, 128, 129])
        op['a'][rows] = 0
        op['res'][rows] = 1000.0 + torch.randn(rows.numel(), D, generator=G.gen(8))
        _res_ln_once(gpu, 'wide', M, K, kmajor=True, eps=eps, op=op, what=f'offset rows eps {eps:g} sched {sched}')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('period', (64, 197))
def test_gemm_res_ln_periodic(gpu, period, family):
    """sf_gemm_res_ln768_periodic: X[m] = A[m] W^T + bias + R[m % period] with the minimum period 64 (a 64-row wave tile wraps at most once) and 197,
    M = 3 period + 17 (the table wraps inside tiles and at a ragged tail), both weight layouts, the table strided (ldr = 772).  The periodic launcher has no
    schedule hook: it runs round 2's loop when K % 64 != 0 or K < 128 and the quadrant-phased one otherwise, so K = 96 and K = 128 reach both."""
    M = 3 * period + 17
    for K in (96, 128):
        op = dict(_ops(family, M, D, K))
        op['res'] = op['res'][:period].contiguous()
        for kmajor in (False, True):
            _res_ln_once(gpu, family, M, K, kmajor=kmajor, period=period, ldr=772, op=op, what=f'period {period} kmajor={int(kmajor)}', kernel='sf_gemm_res_ln768_periodic')


# =====================================================================================================================================================
# 5. sf_gemm_mxfp8 / sf_gemm_mx_res_ln768: operands built directly as e4m3 bytes and E8M0 scale planes (the quantiser is not involved)
# =====================================================================================================================================================
@contextlib.contextmanager
def _mx_sched(sched):
    from synchformer_amd import _lib
    lib = _lib.load()
    lib.sf_gemm_mx_force_schedule(sched)
    try:
        yield
    finally:
        lib.sf_gemm_mx_force_schedule(-1)


def _mx_device_operands(op, dev, pad, a_tile=256):
    """Device views of MXFP8 operands: bytes as column slices (row stride K + pad, rows beyond M 0x7F), scale planes with more rows than whole tiles need
    (the extra rows 0xFF)."""
    M, N, K = op['M'], op['N'], op['K']
    aq = _place(op['aq'], K + pad, 0, dev, rows=M + 3) if pad else torch.cat([op['aq'], torch.full((3, K), 0x7F, dtype=U8)]).to(dev)
    wq = _place(op['wq'], K + pad, 0, dev) if pad else op['wq'].to(dev)
    asc = G.mx_planes(op['asc'], -(-M // a_tile) * a_tile + 8, fill=0xFF).to(dev)
    wsc = G.mx_planes(op['wsc'], -(-N // 256) * 256 + 8, fill=0xFF).to(dev)
    return aq, asc, wq, wsc


MX_EPILOGUES = (  # out dtype, gelu, res, bias: all eight {fp32, bf16} x {GELU} x {residual}, the fp32 residual in place and in its own buffer
    (F32, False, None, True), (F32, False, 'inplace', True), (F32, False, 'separate', False), (F32, True, None, False), (F32, True, 'inplace', True),
    (BF16, False, None, True), (BF16, False, None, False), (BF16, False, 'separate', False), (BF16, True, None, True), (BF16, True, 'separate', True))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('K,sched', [(128, 0), (256, 0), (256, 1), (384, 0), (512, 0), (512, 1)])
def test_gemm_mxfp8(gpu, K, sched, family):
    """sf_gemm_mxfp8 at K = 128 .. 512 (nk = 1 .. 4 of the 128-deep stages; the quadrant-phased schedule where K % 256 == 0), M = 1, 255, 257, N = 64, 192, 320,
    lda = ldw = K + 16, fp32 / bf16 outputs with bias, GELU, in-place and separate residual (ldr = N + 12); the reference is the float64 product of the
    dequantised operands."""
    from synchformer_amd import ops
    with _mx_sched(sched):
        for M in (1, 255, 257):
            for N in (64, 192, 320):
                op = G.mx_operands(family, M, N, K, seed=M * 1009 + N * 7 + K + (family == 'wide'))
                aq, asc, wq, wsc = _mx_device_operands(op, gpu, 16)
                extra = G.mx_group_term(op['a'], op['w']) if family == 'wide' else None
                for dtype, gelu, res, bias in MX_EPILOGUES:
                    out = _Out(gpu, M, N, dtype, ld=N + 8, off=8, init=op['res'] if res == 'inplace' else None)
                    r = out.view if res == 'inplace' else (_place(op['res'], N + 12, 4, gpu, rows=M + 3) if res == 'separate' else None)
                    ops.gemm_mxfp8(aq, asc, wq, wsc, op['bias'].to(gpu) if bias else None, out.view, M=M, residual=r, gelu=gelu)
                    b = op['bias'] if bias else None
                    pre, S = G.reference(op['a'], op['w'], b)
                    rr = op['res'] if res else None
                    exp = G.expected(pre, S, rr, gelu=gelu, out_bf16=dtype == BF16, d=G.depth(K, '32x32x64'), exact_pre=family == 'exact', extra=extra)
                    emu = G.emulate(op['a'], op['w'], b, rr, gelu=gelu, out_bf16=dtype == BF16) if (family == 'wide' or gelu) else None
                    _verify('sf_gemm_mxfp8', f'{M}x{N}x{K} sched {sched} {dtype} gelu={int(gelu)} res={res}', family, out.get(), exp, emu, dtype == BF16, gelu)


@pytest.mark.parametrize('K,sched', [(128, 0), (256, 1), (384, 0), (512, 1)])
def test_gemm_mxfp8_mx_output(gpu, K, sched):
    """The MXFP8 output (N % 128 == 0; N = 256, M = 255 and 257) in the `exact` family: bytes and scale planes equal the OCP quantisation of the bf16-rounded exact
    result, byte for byte; rows beyond M of the bytes and of every scale plane keep their canary."""
    from synchformer_amd import ops
    N = 256
    with _mx_sched(sched):
        for M in (255, 257):
            op = G.mx_operands('exact', M, N, K, seed=M + K)
            aq, asc, wq, wsc = _mx_device_operands(op, gpu, 16)
            out = _Out(gpu, M, N, U8, ld=N + 16, off=16)
            sc_pre = G.canary((N // 128, M + 5, 4), U8)
            sc = sc_pre.to(gpu)
            ops.gemm_mxfp8(aq, asc, wq, wsc, op['bias'].to(gpu), out.view, M=M, out_scales=sc)
            pre, _ = G.reference(op['a'], op['w'], op['bias'])
            q_ref, s_ref = G.mx_quant_ref(pre.float().bfloat16())
            got_q, got_s = out.get(), sc.cpu()
            assert torch.equal(got_s[:, M:], sc_pre[:, M:]), 'scale rows beyond M were written'
            assert torch.equal(G.mx_unplane(got_s, M), s_ref), 'scale bytes'
            assert torch.equal(got_q, q_ref), 'element bytes'


def _mx_res_ln_once(dev, family, M, K, *, strided=False, what=''):
    """One sf_gemm_mx_res_ln768 launch: X as a GEMM output (d = K / 64 + 64, c = 2); the dequantised (Y, sY) against the float64 LayerNorm of the float64 X under
    the LayerNorm bar + the quantiser's own step: one e4m3 step of the block (2^-3 of the block maximum's power of two), two for an element that may saturate
    (|y| >= 1.75 of that power of two: the block maximum lands in [256, 512) and saturates at 448).  No byte-mismatch share: every element is compared."""
    from synchformer_amd import ops
    op = G.mx_operands(family, M, D, K, seed=M * 13 + K + (family == 'wide'))
    gamma, beta = _ln_params(K + M)
    aq, asc, wq, wsc = _mx_device_operands(op, dev, 16 if strided else 0, a_tile=128)
    x = _Out(dev, M, D, F32, ld=776 if strided else D, off=8 if strided else 0, init=None if strided else op['res'])
    r = _place(op['res'], 772, 4, dev, rows=M + 1) if strided else None
    yq = _Out(dev, M, D, U8, ld=784 if strided else D, off=16 if strided else 0)
    sy_pre = G.canary((6, M + 5, 4), U8)
    sy = sy_pre.to(dev)
    ops.gemm_mx_res_ln(aq, asc, wq, wsc, op['bias'].to(dev), x.view, gamma.to(dev), beta.to(dev), yq.view, sy, 1e-6, M=M, residual=r)
    pre, S = G.reference(op['a'], op['w'], op['bias'])
    extra = None
    if family == 'wide':                                            # (on the device for the tall case: M * 768 * K products to look at)
        where = dev if M > 1024 else 'cpu'
        extra = G.mx_group_term(op['a'].to(where), op['w'].to(where)).cpu()
    exp = G.expected(pre, S, op['res'], gelu=False, out_bf16=False, d=G.depth(K, '32x32x64'), exact_pre=family == 'exact', extra=extra)
    emu = G.emulate(op['a'], op['w'], op['bias'], op['res'], gelu=False, out_bf16=False) if family == 'wide' else None
    _verify('sf_gemm_mx_res_ln768', f'X {M}x{K} {what}', family, x.get(), exp, emu, False)
    got_q, got_s = yq.get(), sy.cpu()
    assert torch.equal(got_s[:, M:], sy_pre[:, M:]), 'scale rows beyond M were written'
    yref, ybar = G.layernorm64(exp['ref'], gamma, beta, 1e-6, exp['bar'])
    amax = (yref.abs() + ybar).view(M, 24, 32).amax(-1).clamp_min(2.0 ** -126)
    p2 = torch.exp2(torch.floor(torch.log2(amax))).repeat_interleave(32, 1)
    qbar = torch.where(yref.abs() + ybar >= 1.75 * p2, 2.0 ** -2 * p2, 2.0 ** -3 * p2)
    err = (G.mx_dequant(got_q, G.mx_unplane(got_s, M)) - yref).abs()
    worst = float((err / (ybar + qbar)).max())
    _record('sf_gemm_mx_res_ln768', f'{family} Y {M}x{K} {what}', worst, 0.0)
    bad = ~(err <= ybar + qbar)
    assert not bad.any(), f'sf_gemm_mx_res_ln768 Y {M}x{K} {what}: {int(bad.sum())} elements outside the bar (worst {worst:.3g}), first at {bad.nonzero()[0].tolist()}'


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('K', (128, 256, 384))
def test_gemm_mx_res_ln(gpu, K, family):
    """K = 128, 256, 384 (nk = 1, 2, 3 stages: the rotation `(blockIdx.x >> 3) % nk & ~1` at an odd nk) at M = 1, 129 and 128 * 48 + 5 (every rotation residue),
    and one strided case (lda = ldw = K + 16, ldr / ldx / ldy = 772 / 776 / 784)."""
    for M in (1, 129, 128 * 48 + 5):
        _mx_res_ln_once(gpu, family, M, K)
    _mx_res_ln_once(gpu, family, 129, K, strided=True, what='strided')


def test_mxfp8_mfma_group_alignment(gpu):
    """What gemm_oracle.mx_group_term rests on, asserted: how v_mfma_scale_f32_32x32x64_f8f6f4 sums one large product next to small ones (through sf_gemm_mxfp8,
    fp32 output, W = 1).  The large product is 448 * 2^7 = 57344 = 1.75 * 2^15 at k = 0.
      - a second product 2^e at k = 1 (same group of 8 k) survives exactly for e >= 2 and is lost entirely for e <= 1: the group is cut below 2^(15 - 13);
      - at k = 40 (the other 32-block of the same 64-deep step) and k = 70 (the next step) it survives down to 2^-8 = one fp32 ulp of 57344 and 2^-9 (half an
        ulp, tie to even) is lost: fp32 behaviour;
      - 31 products 2^e at k = 1 .. 31 and 32 at k = 32 .. 63, e = 1 .. -2: the 7 that share the large product's group are lost, the other 24 + 32 survive -
        the cut is per group of 8, not per 32-block."""
    from synchformer_amd import ops
    M, N, K = 32, 64, 128
    big = 448.0 * 2.0 ** 7

    def f8(x):
        return int(torch.tensor(float(x)).to(torch.float8_e4m3fn).view(U8))

    def run(aq, asc):
        wq, wsc = torch.full((N, K), f8(1.0), dtype=U8), torch.full((N, K // 32), 127, dtype=U8)
        out = torch.zeros(M, N, device=gpu)
        ops.gemm_mxfp8(aq.to(gpu), G.mx_planes(asc, 256).to(gpu), wq.to(gpu), G.mx_planes(wsc, 256).to(gpu), None, out)
        torch.cuda.synchronize()
        return out.cpu()[:, 0].double() - big

    for k_small, e_list, e_lost in ((1, range(15, -3, -1), 1), (40, range(15, -17, -1), -9), (70, range(15, -17, -1), -9)):
        aq, asc = torch.zeros(M, K, dtype=U8), torch.full((M, K // 32), 127, dtype=U8)
        aq[:, 0], asc[:, 0] = f8(448.0), 134
        want = torch.zeros(M, dtype=torch.float64)
        for i, e in enumerate(e_list):
            blk = k_small // 32
            sc = 134 if blk == 0 else max(120, min(134, 127 + e))
            aq[i, k_small], asc[i, blk] = f8(2.0 ** (e - (sc - 127))), sc
            want[i] = 2.0 ** e if e > e_lost else 0.0
        got = run(aq, asc)
        assert torch.equal(got, want), f'second product at k = {k_small}: {got.tolist()} != {want.tolist()}'
    aq, asc = torch.zeros(M, K, dtype=U8), torch.full((M, K // 32), 127, dtype=U8)
    aq[:, 0], asc[:, 0] = f8(448.0), 134
    want = torch.zeros(M, dtype=torch.float64)
    for i, e in enumerate((1, 0, -1, -2)):
        aq[i, 1:32] = f8(2.0 ** (e - 7))
        aq[i, 32:64], asc[i, 1] = f8(1.0), 127 + e
        want[i] = (24 + 32) * 2.0 ** e
    got = run(aq, asc)
    assert torch.equal(got, want), f'63 small products: {got.tolist()} != {want.tolist()}'
