"""GPU: the bandwidth-class kernels around the train-step GEMMs (csrc/sf_train.hip, csrc/sf_rowops.hip) against plain float64 restatements of
the same operations, computed on the host from the very (bf16-rounded) inputs the kernel sees.

Conventions of every test below:
  - outputs that are one fp32 operation followed by a bf16 rounding, and moves (transposes), are compared BIT FOR BIT against torch fp32 + .bfloat16()
    (round-to-nearest-even);
  - reductions are bounded relative to the sum of ABSOLUTE values of their terms: |got - ref| <= (d + c) * u * sum|t| with u = 2^-24 (fp32 unit roundoff) and d
    the longest chain of dependent fp32 additions in the kernel's summation tree (recursive-summation bound gamma_d); cancellation cannot fail a correct
    kernel, a missing or doubled row (one term of size ~ sum|t| / rows) cannot pass;
  - every output buffer is pre-filled with a canary (NaN for fp32, 7.0 / NaN bits for bf16) wherever the kernel must not write, and checked afterwards;
  - accumulate flags run both ways on top of a non-zero prefill; strided operands are column slices of wider buffers (row stride > logical width).
Every launch stays inside its header contract (16-byte aligned rows where the kernel does 16-byte accesses)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # fp32 unit roundoff
D = 768


def _lib():
    from synchformer_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from synchformer_amd import _lib as L
    L.check(rc, what)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def _assert_bits(got, ref, what):
    g, r = _bits(got.cpu()), _bits(ref.cpu())
    bad = g != r
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} elements differ bitwise, first at {i}: got {got.cpu()[tuple(i)].item()!r} '
                             f'want {ref.cpu()[tuple(i)].item()!r}')


def _assert_within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (all float64 on the host)."""
    got, ref, tol = got.double().cpu(), ref.double().cpu(), torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)                     # NaN in got fails
    if bad.any():
        i = bad.nonzero()[0].tolist()
        ratio = (err / tol.clamp_min(1e-300)).max().item()
        raise AssertionError(f'{what}: {int(bad.sum())} of {ref.numel()} elements outside the bar (worst err / bar = {ratio:.3g}); first at {i}: '
                             f'got {got[tuple(i)].item()!r} want {ref[tuple(i)].item()!r} bar {tol[tuple(i)].item()!r}')


def _map_rows(m, r):
    """ops.rowmap semantics: logical row r -> physical row (r / n12) * sA + ((r % n12) / n2) * s1 + (r % n2) * s2 + off."""
    if m is None:
        return r
    n12, n2, sA, s1, s2, off = m
    return (r // n12) * sA + ((r % n12) // n2) * s1 + (r % n2) * s2 + off


def _bf16_ulp(ref):
    """bf16 spacing at |ref| (float64): 2^(e - 7), e = max(floor(log2 |ref|), -126); subnormal spacing 2^-133 at and below 2^-126."""
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ======================================================================================================================================
# 1. LayerNorm(768) backward: sf_layernorm768_bwd / sf_layernorm768_bwd_bf16
# ======================================================================================================================================
def _ln_bwd_ref(x, gamma, dy, eps, chunk=8192):
    """fp64 LayerNorm backward of the rows of x (R, 768) with incoming gradient dy (R, 768), both float64 on the host, in row chunks (bounded memory).
    Returns dx, dgamma, dbeta and the per-element / per-column error scales the bars are built from."""
    R = x.shape[0]
    dx = torch.empty(R, D, dtype=torch.float64)
    sdx = torch.empty(R, D, dtype=torch.float64)
    dg, db = torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    sdg, sdb = torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    for r0 in range(0, R, chunk):
        xs, g = x[r0:r0 + chunk], dy[r0:r0 + chunk]
        mu = xs.mean(1, keepdim=True)
        xc = xs - mu
        rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
        xh = xc * rstd
        gd = gamma * g
        a, b = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
        dx[r0:r0 + chunk] = rstd * (gd - a - xh * b)
        amp = 1.0 + rstd * xs.abs().mean(1, keepdim=True)          # the mean's rounding, seen through xhat = (x - mean) * rstd
        sdx[r0:r0 + chunk] = rstd * (gd.abs() + gd.abs().mean(1, keepdim=True) + (xh.abs() + 1.0) * (gd * xh).abs().mean(1, keepdim=True)) * amp
        dg += (g * xh).sum(0)
        db += g.sum(0)
        sdg += (g.abs() * (xh.abs() + rstd * xs.abs().mean(1, keepdim=True))).sum(0)
        sdb += g.abs().sum(0)
    return dx, dg, db, sdx, sdg, sdb


def _ln_rpw(rows):
    return 8 if rows >= 16384 else (2 if rows >= 4096 else 1)     # the kernel's rows-per-wave regimes (layernorm768_bwd_impl)


def _ln_param_depth(rows):
    """Longest chain of fp32 additions behind one dgamma / dbeta column: rpw rows per wave, 2 LDS levels, then colsum_partials_kernel's
    ceil(nblk / 64) + 3 per accumulator, 2 levels, 16 sequential lane groups, + the accumulate add."""
    rpw = _ln_rpw(rows)
    nblk = -(-rows // (4 * rpw))
    return rpw + 2 + -(-nblk // 64) + 3 + 2 + 16 + 1


VIS_L, VIS_P, AGG_V = 1569, 1568, 197          # engine.py: Stage-1 visual segment rows, patch rows, aggregation rows per frame
AUD_L, AUD_P, AGG_A, AUD_NT = 74, 72, 13, 6


def _ln_case(rows, dy_bf16, acc_dx, acc_dp, eps, maps, seed):
    """Host operands of one LayerNorm-backward launch: strided x / dy / dx buffers (dx NaN outside the mapped rows and beyond 768 columns, the prefill on
    the mapped rows when accumulating), the row maps, and the physical rows dx_map writes."""
    from synchformer_amd import ops
    g = _gen(seed)
    if maps == 'visual':                           # stage1.py:421 / :439: patch rows of (n, 1569) segments, dY from the (n * 8, 197) aggregation rows
        n = -(-rows // VIS_P)
        x_map = dx_map = ops.rowmap(VIS_P, VIS_P, VIS_L, 0, 1, 1)
        dy_map = ops.rowmap(VIS_P, 196, 8 * AGG_V, AGG_V, 1, 1)
        x_rows, dy_rows, dx_rows = n * VIS_L, n * 8 * AGG_V, n * VIS_L
    elif maps == 'audio':                          # stage1.py:496 / :518 / :536: tokmap + the frequency-major aggregation map (s2 > s1)
        n = -(-rows // AUD_P)
        x_map = dx_map = ops.rowmap(AUD_P, AUD_P, AUD_L, 0, 1, 2)
        dy_map = ops.rowmap(AUD_P, AUD_NT, AUD_NT * AGG_A, 1, AGG_A, 1)
        x_rows, dy_rows, dx_rows = n * AUD_L, n * AUD_NT * AGG_A, n * AUD_L
    else:
        x_map = dy_map = dx_map = None
        x_rows = dy_rows = dx_rows = rows
    ldx, lddy, lddx = D + 32, (D + 64 if dy_bf16 else D + 16), D + 8            # every operand strided (row stride > 768)
    xw = torch.randn(x_rows, ldx, generator=g) * 2.0 + 0.3
    gamma = torch.randn(D, generator=g) * 0.5 + 1.0
    dyw = torch.randn(dy_rows, lddy, generator=g)
    if dy_bf16:
        dyw = dyw.bfloat16()
    phys = _map_rows(dx_map, torch.arange(rows))
    mapped = torch.zeros(dx_rows, dtype=torch.bool)
    mapped[phys] = True
    dxw = torch.full((dx_rows, lddx), float('nan'))
    pre_dx = torch.randn(rows, D, generator=g)
    if acc_dx:
        dxw[phys, :D] = pre_dx
    pre_p = torch.randn(2, D, generator=g)
    return dict(x_map=x_map, dy_map=dy_map, dx_map=dx_map, xw=xw, gamma=gamma, dyw=dyw, dxw=dxw, phys=phys, mapped=mapped, pre_dx=pre_dx, pre_p=pre_p)


LN_CASES = [
    # rows, dy bf16, acc_dx, acc_dp, eps, maps
    (1, False, False, False, 1e-6, None),
    (3, True, True, True, 1e-12, None),
    (4095, False, True, False, 1e-6, None),        # last rpw = 1 size
    (4096, True, False, True, 1e-6, None),         # first rpw = 2 size
    (4099, False, False, False, 1e-12, None),
    (16383, True, True, True, 1e-6, None),         # last rpw = 2 size
    (16384, False, True, True, 1e-6, None),        # first rpw = 8 size
    (16384 + 37, True, False, False, 1e-12, None),
    (AUD_P * 61, False, True, True, 1e-12, 'audio'),
    (AUD_P * 230, True, False, True, 1e-6, 'audio'),
    (2 * 14 * VIS_L, True, True, False, 1e-6, None),    # 43,932 rows = two Stage-1 clips (the closing norms of the visual blocks: bf16 dY, acc_dx)
    (2 * 14 * VIS_P, False, False, True, 1e-6, 'visual'),   # the visual tower's final norm (stage1.py:439): three row maps
]


@pytest.mark.parametrize('rows,dy_bf16,acc_dx,acc_dp,eps,maps', LN_CASES,
                         ids=[f'{c[0]}-{"bf16" if c[1] else "f32"}-dx{int(c[2])}-dp{int(c[3])}-eps{c[4]:g}-{c[5] or "id"}' for c in LN_CASES])
def test_layernorm768_bwd_vs_fp64(gpu, rows, dy_bf16, acc_dx, acc_dp, eps, maps):
    """sf_layernorm768_bwd / sf_layernorm768_bwd_bf16 at every rows-per-wave regime and its boundaries, both dy dtypes, both accumulate flags on a
    non-zero prefill, identity and Stage-1 row maps, against fp64.
    Bars: dx - the four per-row fp32 reductions (sum x, sum (x - mean)^2, sum g*dy, sum g*dy*xhat) are 12-term lane chains + a 6-level butterfly
    (18 deep), rsqrt adds 1 ulp; all of it enters dx linearly through rstd, xhat and the two means -> |err| <= 64 u * rstd * (|g dy| + mean|g dy| +
    (|xhat| + 1) * mean|g dy xhat|) * (1 + rstd * mean|x|), the last factor for the mean's own rounding seen through xhat; plus 1 ulp of the
    accumulate add.  dgamma / dbeta - column sums over rows, d = _ln_param_depth(rows) deep, each term carrying xhat's ~40 u error -> (d + 64) u *
    sum|dy| (|xhat| + rstd mean|x|) and (d + 2) u sum|dy|, plus 2 u |prefill|.  Rows of dx outside the map and the columns beyond 768 keep their NaN."""
    from synchformer_amd import train as T
    c = _ln_case(rows, dy_bf16, acc_dx, acc_dp, eps, maps, seed=rows + 7 * dy_bf16)
    dev = gpu
    xw, dyw, dxw = c['xw'].to(dev), c['dyw'].to(dev), c['dxw'].to(dev)
    x, dy, dx = xw[:, :D], dyw[:, :D], dxw[:, :D]
    gamma = c['gamma'].to(dev)
    par = torch.full((2 * D + 64,), float('nan'), device=dev)
    dgamma, dbeta = par[:D], par[D + 32:2 * D + 32]                     # NaN canary between and after the two parameter gradients
    if acc_dp:
        dgamma.copy_(c['pre_p'][0])
        dbeta.copy_(c['pre_p'][1])
    ws = torch.empty(2 * D * -(-rows // 4), device=dev)
    T.ln_bwd(x, gamma, dy, dx, dgamma, dbeta, ws, rows, eps, x_map=c['x_map'], dy_map=c['dy_map'], dx_map=c['dx_map'], acc_dx=acc_dx, acc_dp=acc_dp)
    torch.cuda.synchronize()

    rr = torch.arange(rows)
    xin = c['xw'][_map_rows(c['x_map'], rr), :D].double()
    dyin = c['dyw'][_map_rows(c['dy_map'], rr), :D].double()
    rdx, rdg, rdb, sdx, sdg, sdb = _ln_bwd_ref(xin, c['gamma'].double(), dyin, eps)
    got = dxw.cpu()
    tol = 64 * U32 * sdx
    if acc_dx:
        rdx = rdx + c['pre_dx'].double()
        tol = tol + 2 * U32 * rdx.abs()
    _assert_within(got[c['phys'], :D], rdx, tol, 'dx')
    assert torch.isnan(got[~c['mapped']]).all(), 'dx rows outside the row map were written'
    assert torch.isnan(got[:, D:]).all(), 'dx columns beyond 768 were written'
    d = _ln_param_depth(rows)
    pg, pb = c['pre_p'].double() if acc_dp else torch.zeros(2, D, dtype=torch.float64)
    pc = par.cpu()
    _assert_within(pc[:D], rdg + pg, (d + 64) * U32 * sdg + 2 * U32 * pg.abs(), 'dgamma')
    _assert_within(pc[D + 32:2 * D + 32], rdb + pb, (d + 2) * U32 * sdb + 2 * U32 * pb.abs(), 'dbeta')
    assert torch.isnan(pc[D:D + 32]).all() and torch.isnan(pc[2 * D + 32:]).all(), 'writes beyond dgamma / dbeta'


# ======================================================================================================================================
# 2. sf_layernorm768_bwd_branch against fp64 (not only against the two-launch path)
# ======================================================================================================================================
BRANCH_LN_CASES = [
    # rows, dy bf16, acc_dx, seq_rows, scales kind
    (3 * VIS_L, False, True, VIS_L, 'mixed'),          # rpw = 2: 8-row blocks, 1569 % 8 = 1 -> every sequence edge falls inside a block
    (11 * VIS_L, True, True, VIS_L, 'mixed'),          # rpw = 8: 32-row blocks straddle the edges
    (4099, True, False, 1, None),                      # no stochastic depth on the next branch (seq_scale NULL)
    (5 * 197 + 3, False, False, 197, 'mixed'),
]


@pytest.mark.parametrize('rows,dy_bf16,acc_dx,seq_rows,scales', BRANCH_LN_CASES,
                         ids=[f'{c[0]}-{"bf16" if c[1] else "f32"}-dx{int(c[2])}-L{c[3]}-{c[4] or "noscale"}' for c in BRANCH_LN_CASES])
def test_layernorm768_bwd_branch_vs_fp64(gpu, rows, dy_bf16, acc_dx, seq_rows, scales):
    """sf_layernorm768_bwd_branch: dx / dgamma / dbeta as sf_layernorm768_bwd (same bars, test above); y_next = bf16(scale[r // seq_rows] * dx_final)
    bit-exact against torch fp32 + RNE on the kernel's own dx (one fp32 multiply, one rounding; a dropped sequence, scale 0, gives 0 * dx with its sign, as
    the kernel multiplies); dbias_next = the fp64 column sum of scale[r // seq_rows] * dx_final, bar (d + 2) u sum|scale dx| with d the LayerNorm
    parameter depth (same two-stage tree).  Scale vectors hold 0 and values other than 1; y_next is strided with canary columns and canary rows after."""
    lib = _lib()
    g = _gen(100 + rows)
    dev = gpu
    ldx, lddy, lddx, ldyn = D + 32, D + 64, D + 16, D + 24
    xw = (torch.randn(rows, ldx, generator=g) * 2.0 - 0.2).to(dev)
    gamma = (torch.randn(D, generator=g) * 0.5 + 1.0).to(dev)
    dyw = torch.randn(rows, lddy, generator=g)
    dyw = (dyw.bfloat16() if dy_bf16 else dyw).to(dev)
    pre_dx = torch.randn(rows, D, generator=g)
    dxw = torch.full((rows, lddx), float('nan'))
    if acc_dx:
        dxw[:, :D] = pre_dx
    dxw = dxw.to(dev)
    n_seq = -(-rows // seq_rows)
    sc = None
    if scales:
        sc = torch.tensor([(0.0, 1.25, 0.8, 1.0 / 0.9)[i % 4] for i in range(n_seq)], dtype=torch.float32).to(dev)
    ynw = torch.full((rows + 3, ldyn), 7.0, dtype=torch.bfloat16, device=dev)
    par = torch.full((3 * D + 96,), float('nan'), device=dev)
    dgamma, dbeta, dbn = par[:D], par[D + 32:2 * D + 32], par[2 * D + 64:3 * D + 64]
    ws = torch.empty(3 * D * -(-rows // 4), device=dev)
    _ok(lib.sf_layernorm768_bwd_branch(xw.data_ptr(), ldx, gamma.data_ptr(), dyw.data_ptr(), 1 if dy_bf16 else 0, lddy, dxw.data_ptr(), lddx, int(acc_dx),
                                       dgamma.data_ptr(), dbeta.data_ptr(), 0, ynw.data_ptr(), ldyn, sc.data_ptr() if sc is not None else None, seq_rows,
                                       dbn.data_ptr(), ws.data_ptr(), rows, 1e-6, _st()), 'sf_layernorm768_bwd_branch')
    torch.cuda.synchronize()
    rdx, rdg, rdb, sdx, sdg, sdb = _ln_bwd_ref(xw.cpu()[:, :D].double(), gamma.cpu().double(), dyw.cpu()[:, :D].double(), 1e-6)
    tol = 64 * U32 * sdx
    if acc_dx:
        rdx = rdx + pre_dx.double()
        tol = tol + 2 * U32 * rdx.abs()
    dxg = dxw.cpu()
    _assert_within(dxg[:, :D], rdx, tol, 'dx')
    assert torch.isnan(dxg[:, D:]).all(), 'dx columns beyond 768 were written'
    d = _ln_param_depth(rows)
    pc = par.cpu()
    _assert_within(pc[:D], rdg, (d + 64) * U32 * sdg, 'dgamma')
    _assert_within(pc[D + 32:2 * D + 32], rdb, (d + 2) * U32 * sdb, 'dbeta')
    s_row = sc.cpu()[torch.arange(rows) // seq_rows] if sc is not None else torch.ones(rows)
    dxf = dxg[:, :D]
    yref = (dxf * s_row[:, None]).bfloat16()
    yn = ynw.cpu()
    _assert_bits(yn[:rows, :D], yref, 'y_next')
    assert (yn[:rows, D:].float() == 7.0).all() and (yn[rows:].float() == 7.0).all(), 'y_next written outside (rows, 768)'
    sdx_ = dxf.double() * s_row.double()[:, None]
    _assert_within(pc[2 * D + 64:3 * D + 64], sdx_.sum(0), (d + 2) * U32 * sdx_.abs().sum(0), 'dbias_next')
    assert torch.isnan(pc[D:D + 32]).all() and torch.isnan(pc[2 * D + 32:2 * D + 64]).all() and torch.isnan(pc[3 * D + 64:]).all(), 'parameter canaries'


# ======================================================================================================================================
# 3. sf_branch_grad
# ======================================================================================================================================
BRANCH_CASES = [
    # rows, cols, seq_rows (None = no seq_scale), accumulate
    (3000, D, None, False),
    (3000, D, None, True),
    (200 * 90 + 17, D, 200, True),        # rows >= 16384 with seq_rows < 256: rpb drops from 256 to 64
    (64 * 300 + 5, 96, 64, False),        # the shortest supported sequence, a width that is a multiple of 32 but not of 64
    (12 * VIS_L, D, VIS_L, True),         # rpb = 256 blocks straddling 1569-row sequence edges
    (2 * VIS_L + 100, D, VIS_L, False),   # rpb = 64, a partial last sequence
]


@pytest.mark.parametrize('rows,cols,seq_rows,acc', BRANCH_CASES, ids=[f'{c[0]}x{c[1]}-L{c[2]}-acc{int(c[3])}' for c in BRANCH_CASES])
def test_branch_grad_vs_fp64(gpu, rows, cols, seq_rows, acc):
    """sf_branch_grad: y = bf16(s[r // seq_rows] * dx) bit-exact against torch fp32 + RNE (a dropped sequence is written as +0: the kernel does not read it);
    dbias (=|+=) fp64 column sums of s * dx.  Bar: the block's 32 row lanes sum rpb / 32 <= 8 rows each, 3 shuffle levels, 2 LDS levels, then the
    colsum_partials tree (ceil(nblk / 64) + 3, 2, 16) and the accumulate add: d <= 8 + 3 + 2 + ceil(nblk / 64) + 3 + 2 + 16 + 1; products are exact in fp32
    up to 1 rounding -> (d + 1) u sum|s dx| + 2 u |prefill|.  dx is a column slice of a wider buffer; y is strided with canary columns and rows."""
    lib = _lib()
    g = _gen(rows + cols)
    dev = gpu
    ldx, ldy = cols + 36, cols + 20
    dxw = torch.randn(rows, ldx, generator=g)
    dx_h = dxw[:, 4:4 + cols]                                       # 16-byte aligned column slice
    n_seq = -(-rows // seq_rows) if seq_rows else 0
    sc = torch.tensor([(1.25, 0.0, 0.8, 1.0 / 0.9)[i % 4] for i in range(n_seq)], dtype=torch.float32) if seq_rows else None
    yw = torch.full((rows + 2, ldy), 7.0, dtype=torch.bfloat16, device=dev)
    pre = torch.randn(cols, generator=g)
    db = torch.full((cols + 8,), float('nan'), device=dev)
    if acc:
        db[:cols] = pre.to(dev)
    ws = torch.empty(cols * -(-rows // 64), device=dev)
    dxd = dxw.to(dev)
    scd = sc.to(dev) if sc is not None else None                  # (device tensors live in names: a freed temporary's block is reused by the next copy)
    _ok(lib.sf_branch_grad(dxd[:, 4:].data_ptr(), ldx, scd.data_ptr() if scd is not None else None, seq_rows or 1, yw.data_ptr(), ldy, rows, cols,
                           db.data_ptr(), int(acc), ws.data_ptr(), _st()), 'sf_branch_grad')
    torch.cuda.synchronize()
    s_row = sc[torch.arange(rows) // seq_rows] if sc is not None else torch.ones(rows)
    scaled = torch.where(s_row[:, None] == 0, torch.zeros(()), dx_h * s_row[:, None])
    y = yw.cpu()
    _assert_bits(y[:rows, :cols], scaled.bfloat16(), 'y')
    assert (y[:rows, cols:].float() == 7.0).all() and (y[rows:].float() == 7.0).all(), 'y written outside (rows, cols)'
    rpb = 256 if rows >= 16384 else 64
    if seq_rows and rpb > seq_rows:
        rpb = 64
    nblk = -(-rows // rpb)
    d = 8 + 3 + 2 + -(-nblk // 64) + 3 + 2 + 16 + 1
    ref = scaled.double().sum(0) + (pre.double() if acc else 0.0)
    tol = (d + 1) * U32 * scaled.double().abs().sum(0) + (2 * U32 * pre.double().abs() if acc else 0.0)
    dbc = db.cpu()
    _assert_within(dbc[:cols], ref, tol, 'dbias')
    assert torch.isnan(dbc[cols:]).all(), 'dbias written beyond cols'


# ======================================================================================================================================
# 4. sf_add_scale_ln768
# ======================================================================================================================================
@pytest.mark.parametrize('rows,seq_rows', [(1001, None), (3 * 197 + 2, 197), (4 * 1569 + 3, 1569)], ids=['noscale-1001', 'L197-593', 'L1569-6279'])
def test_add_scale_ln768_vs_fp64(gpu, rows, seq_rows):
    """sf_add_scale_ln768: x = residual + s[r // seq_rows] * branch and y = bf16(LayerNorm(x) * gamma + beta).
    x bar: one product and one sum in fp32 (or one fused multiply-add, if the compiler contracts them): |err| <= u |s b| + u |x| - at most 1 fp32 ulp of x
    when fused, and exactly 0 for a dropped branch (x == residual).  y bar: 1 bf16 ulp of the fp64 value (half an ulp for the final rounding, the other
    half for fp32 error pushing a value across a rounding boundary) + the fp32 error itself, 64 u (|xhat g| + |b|) by the LayerNorm reductions' depth (see
    test_layernorm768_bwd_vs_fp64).  branch / residual / y are strided slices, rows are not a multiple of 4 (a partial last block of 4 waves), the scale
    vector holds zeros; x and y carry canary rows after and y canary columns."""
    lib = _lib()
    g = _gen(rows)
    dev = gpu
    ldb, ldr, ldx, ldy = D + 40, D + 12, D, D + 16
    bw = torch.randn(rows, ldb, generator=g)
    rw = torch.randn(rows, ldr, generator=g) * 1.5 + 0.4
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1.0, torch.randn(D, generator=g) * 0.2
    n_seq = -(-rows // seq_rows) if seq_rows else 0
    sc = torch.tensor([(0.0, 1.25, 1.0 / 0.85)[i % 3] for i in range(n_seq)], dtype=torch.float32) if seq_rows else None
    xo = torch.full((rows + 3, ldx), float('nan'), device=dev)
    yo = torch.full((rows + 3, ldy), 7.0, dtype=torch.bfloat16, device=dev)
    bd, rd, gd_, bd_ = bw.to(dev), rw.to(dev), gamma.to(dev), beta.to(dev)
    scd = sc.to(dev) if sc is not None else None
    _ok(lib.sf_add_scale_ln768(bd[:, 8:].data_ptr(), ldb, scd.data_ptr() if scd is not None else None, seq_rows or 1, rd[:, 4:].data_ptr(), ldr,
                               xo.data_ptr(), ldx, gd_.data_ptr(), bd_.data_ptr(), yo.data_ptr(), ldy, rows, 1e-6, _st()), 'sf_add_scale_ln768')
    torch.cuda.synchronize()
    br, res = bw[:, 8:8 + D].double(), rw[:, 4:4 + D].double()
    s_row = (sc[torch.arange(rows) // seq_rows] if sc is not None else torch.ones(rows)).double()[:, None]
    xref = res + s_row * br
    xg = xo.cpu()
    prod = (s_row * br).float().double().abs()
    _assert_within(xg[:rows], xref, U32 * prod + U32 * xref.abs(), 'x')
    if sc is not None:
        dropped = (s_row[:, 0] == 0)
        assert torch.equal(xg[:rows][dropped], rw[:, 4:4 + D][dropped]), 'a dropped branch changed the residual'
    assert torch.isnan(xg[rows:]).all(), 'x rows beyond `rows` were written'
    mu = xref.mean(1, keepdim=True)
    xc = xref - mu
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + 1e-6)
    xhg = xc * rstd * gamma.double()
    yref = xhg + beta.double()
    yg = yo.cpu()
    _assert_within(yg[:rows, :D], yref, _bf16_ulp(yref) + 64 * U32 * (xhg.abs() + beta.double().abs()), 'y')
    assert (yg[:rows, D:].float() == 7.0).all() and (yg[rows:].float() == 7.0).all(), 'y written outside (rows, 768)'


# ======================================================================================================================================
# 5. sf_scale_seq_add and sf_scale_rows_map
# ======================================================================================================================================
@pytest.mark.parametrize('form', ['no_residual', 'residual', 'in_place'])
@pytest.mark.parametrize('cols', [D, 96])
def test_scale_seq_add_vs_fp64(gpu, form, cols):
    """sf_scale_seq_add: y = (residual or 0) + s[r // seq_rows] * x.  Without a residual the result is one fp32 product: exact against torch fp32 (a dropped
    sequence is +0, not read).  With one: bar u |s x| + u |y| (product and sum, or one contracted multiply-add), dropped sequences leave the residual
    bit-exact.  In place: y aliases residual.  x is a strided column slice; rows straddle sequence edges; y carries canary columns and rows."""
    lib = _lib()
    dev = gpu
    rows, seq_rows = 3 * 197 + 50, 197
    g = _gen(cols + len(form))
    ldx, ldr = cols + 12, cols + 8
    xw = torch.randn(rows, ldx, generator=g)
    x_h = xw[:, 4:4 + cols]
    sc = torch.tensor([1.25, 0.0, 0.7, 1.0 / 0.9], dtype=torch.float32)
    s_row = sc[torch.arange(rows) // seq_rows][:, None]
    res_h = torch.randn(rows, cols, generator=g)
    if form == 'in_place':
        yw = torch.full((rows + 2, ldr), float('nan'))
        yw[:rows, :cols] = res_h
        yw = yw.to(dev)
        rptr, ldr_ = yw.data_ptr(), ldr
        ldy = ldr
    else:
        ldy = cols + 16
        yw = torch.full((rows + 2, ldy), float('nan'), device=dev)
        rw = torch.full((rows, ldr), float('nan'))
        rw[:, :cols] = res_h
        rd = rw.to(dev)
        rptr, ldr_ = (rd.data_ptr(), ldr) if form == 'residual' else (None, 0)
    xd = xw.to(dev)
    scd = sc.to(dev)
    _ok(lib.sf_scale_seq_add(xd[:, 4:].data_ptr(), ldx, scd.data_ptr(), seq_rows, rptr, ldr_, yw.data_ptr(), ldy, rows, cols, _st()), 'sf_scale_seq_add')
    torch.cuda.synchronize()
    yg = yw.cpu()
    prod = torch.where(s_row == 0, torch.zeros(()), x_h * s_row)
    if form == 'no_residual':
        _assert_bits(yg[:rows, :cols], prod, 'y')
    else:
        ref = res_h.double() + s_row.double() * x_h.double()
        _assert_within(yg[:rows, :cols], ref, U32 * prod.double().abs() + U32 * ref.abs(), 'y')
        dropped = (s_row[:, 0] == 0)
        assert torch.equal(yg[:rows, :cols][dropped], res_h[dropped]), 'a dropped sequence changed the residual'
    assert torch.isnan(yg[:, cols:]).all() and torch.isnan(yg[rows:]).all(), 'y written outside (rows, cols)'


def test_scale_rows_map_forward_and_backward(gpu):
    """sf_scale_rows_map in the two uses of the Stage-2 trainer.  Forward (train.py:442): the input norm's rows, scaled per token, accumulated into the
    token matrix through the segment's token map on top of the positional table - bar u |s x| + u |y| on mapped rows, every other row (OFF / MOD tokens, the
    other modality) bit-unchanged.  Backward (train.py:581): y[r] = s[r] * dx[tokmap(r)], overwrite, one fp32 product: exact (+0 for a dropped token);
    canary rows after y."""
    from synchformer_amd import ops
    lib = _lib()
    dev = gpu
    g = _gen(5)
    B, Sv, Sa = 3, 14, 48
    L = 1 + Sv + 1 + Sa
    table = torch.randn(B * L, D, generator=g)
    for tag, n_tok, off in (('v', Sv, 1), ('a', Sa, 2 + Sv)):
        n = B * n_tok
        tokmap = ops.rowmap(n_tok, n_tok, L, 0, 1, off)
        x_h = torch.randn(n, D, generator=g)
        sc = torch.where(torch.rand(n, generator=g) < 0.3, torch.zeros(()), torch.full((), 1.0 / 0.7))
        y = table.to(dev)
        xd, scd = x_h.to(dev), sc.to(dev)
        _ok(lib.sf_scale_rows_map(xd.data_ptr(), D, None, scd.data_ptr(), y.data_ptr(), D, ops._map(tokmap), n, D, 1, _st()), 'sf_scale_rows_map')
        torch.cuda.synchronize()
        phys = _map_rows(tokmap, torch.arange(n))
        ref = table.double().clone()
        ref[phys] += sc.double()[:, None] * x_h.double()
        yg = y.cpu()
        prod = (sc[:, None] * x_h).double().abs()
        _assert_within(yg[phys], ref[phys], U32 * prod + U32 * ref[phys].abs(), f'{tag} forward')
        other = torch.ones(B * L, dtype=torch.bool)
        other[phys] = False
        assert torch.equal(yg[other], table[other]), f'{tag} forward: rows outside the token map changed'
        dxt = torch.randn(B * L, D, generator=g)
        dln = torch.full((n + 2, D), float('nan'), device=dev)
        dxd = dxt.to(dev)
        _ok(lib.sf_scale_rows_map(dxd.data_ptr(), D, ops._map(tokmap), scd.data_ptr(), dln.data_ptr(), D, None, n, D, 0, _st()), 'sf_scale_rows_map')
        torch.cuda.synchronize()
        want = torch.where(sc[:, None] == 0, torch.zeros(()), dxt[phys] * sc[:, None])
        dg = dln.cpu()
        _assert_bits(dg[:n], want, f'{tag} backward')
        assert torch.isnan(dg[n:]).all(), f'{tag} backward: rows beyond n were written'


# ======================================================================================================================================
# 6. sf_wgrad_sum, sf_seqsum, sf_rowsum_bf16
# ======================================================================================================================================
@pytest.mark.parametrize('split', [1, 2, 3, 4, 5, 7, 27])
@pytest.mark.parametrize('bias', ['none', 'overwrite', 'accumulate'])
def test_wgrad_sum_vs_fp64(gpu, split, bias):
    """sf_wgrad_sum: dw = sum of `split` planes, db (=|+=) sum of `split` bias rows; split covers the unrolled-by-4 loop and its remainder.  n_w is not a
    multiple of 1024 (a partial last block, and the weight / bias boundary inside a block).  Bar: one accumulator chain of split / 4 + (split % 4) terms,
    then 2 levels (+ 1 accumulate add): (split + 4) u sum|part| (+ 2 u |prefill|).  dw / db carry a NaN canary after their last element."""
    lib = _lib()
    dev = gpu
    g = _gen(split * 3 + len(bias))
    n_w, n_b = 4 * (256 * 5 + 3), 772
    part = torch.randn(split, n_w, generator=g)
    bpart = torch.randn(split, n_b, generator=g)
    pre = torch.randn(n_b, generator=g)
    dw = torch.full((n_w + 8,), float('nan'), device=dev)
    db = torch.full((n_b + 8,), float('nan'), device=dev)
    if bias == 'accumulate':
        db[:n_b] = pre.to(dev)
    pd, bd = part.to(dev), bpart.to(dev)
    _ok(lib.sf_wgrad_sum(pd.data_ptr(), n_w, split, dw.data_ptr(), bd.data_ptr() if bias != 'none' else None, n_b, db.data_ptr() if bias != 'none' else None,
                         int(bias == 'accumulate'), _st()), 'sf_wgrad_sum')
    torch.cuda.synchronize()
    dwc, dbc = dw.cpu(), db.cpu()
    _assert_within(dwc[:n_w], part.double().sum(0), (split + 4) * U32 * part.double().abs().sum(0), 'dw')
    assert torch.isnan(dwc[n_w:]).all(), 'dw written beyond n_w'
    if bias == 'none':
        assert torch.isnan(dbc).all(), 'db written without bias partials'
    else:
        acc = bias == 'accumulate'
        ref = bpart.double().sum(0) + (pre.double() if acc else 0.0)
        tol = (split + 4) * U32 * bpart.double().abs().sum(0) + (2 * U32 * pre.double().abs() if acc else 0.0)
        _assert_within(dbc[:n_b], ref, tol, 'db')
        assert torch.isnan(dbc[n_b:]).all(), 'db written beyond n_b'


SEQSUM_CASES = [
    # n_seq, L, cols, row stride, accumulate
    (1, 13, 7, 7, False),            # n_seq = 1: a copy; L * cols = 91
    (5, 13, 7, 12, True),            # row stride > cols, accumulate
    (28, 1569, 768, 768, False),     # the token-table gradient of the visual tower (stage1.py:462)
    (8, 196, 768, 768, True),        # the positional-table call of stage1.py:464 (gtab[1:], sum over frames), here accumulating
    (3, 197, 100, 136, False),       # L * cols = 19700, not a multiple of 256
]


@pytest.mark.parametrize('n_seq,L,cols,ldx,acc', SEQSUM_CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}-ld{c[3]}-acc{int(c[4])}' for c in SEQSUM_CASES])
def test_seqsum_vs_fp64(gpu, n_seq, L, cols, ldx, acc):
    """sf_seqsum: out[l, c] (=|+=) sum_b x[b * L + l, c] - one sequential chain of n_seq terms (+ the accumulate add): bar (n_seq + 1) u sum|x| + 2 u |prefill|;
    n_seq = 1 is exact.  The input starts one row into its buffer (gtab[1:] of stage1.py:464); out carries a NaN canary after L * cols."""
    lib = _lib()
    dev = gpu
    g = _gen(n_seq * L + cols)
    xw = torch.randn(n_seq * L + 1, ldx, generator=g)
    x_h = xw[1:, :cols].reshape(n_seq, L, cols)
    pre = torch.randn(L * cols, generator=g)
    out = torch.full((L * cols + 5,), float('nan'), device=dev)
    if acc:
        out[:L * cols] = pre.to(dev)
    xd = xw.to(dev)
    _ok(lib.sf_seqsum(xd[1:].data_ptr(), ldx, n_seq, L, cols, out.data_ptr(), int(acc), _st()), 'sf_seqsum')
    torch.cuda.synchronize()
    oc = out.cpu()
    ref = x_h.double().sum(0).reshape(-1) + (pre.double() if acc else 0.0)
    if n_seq == 1 and not acc:
        _assert_bits(oc[:L * cols], x_h.reshape(-1), 'out (copy)')
    tol = (n_seq + 1) * U32 * x_h.double().abs().sum(0).reshape(-1) + (2 * U32 * pre.double().abs() if acc else 0.0)
    _assert_within(oc[:L * cols], ref, tol, 'out')
    assert torch.isnan(oc[L * cols:]).all(), 'out written beyond L * cols'


@pytest.mark.parametrize('cols,ldx', [(8, 8), (512, 512), (520, 528), (4992, 5000)])
@pytest.mark.parametrize('acc', [False, True])
def test_rowsum_bf16_vs_fp64(gpu, cols, ldx, acc):
    """sf_rowsum_bf16: out[r] (=|+=) sum_c x[r, c] over a bf16 matrix (exact in fp32 term by term).  One wave per row: two accumulators per lane of
    4 * ceil(cols / 512) terms, 1 add, a 6-level butterfly, the accumulate add -> bar (4 ceil(cols / 512) + 8) u sum|x| + 2 u |prefill|.  Row strides beyond
    cols hold huge values that must not enter the sum; out carries a NaN canary after the last row."""
    lib = _lib()
    dev = gpu
    rows = 37
    g = _gen(cols + acc)
    xw = torch.randn(rows, ldx, generator=g) * 3.0
    xw[:, cols:] = 1e30
    xw = xw.bfloat16()
    pre = torch.randn(rows, generator=g)
    out = torch.full((rows + 4,), float('nan'), device=dev)
    if acc:
        out[:rows] = pre.to(dev)
    xd = xw.to(dev)
    _ok(lib.sf_rowsum_bf16(xd.data_ptr(), ldx, rows, cols, out.data_ptr(), int(acc), _st()), 'sf_rowsum_bf16')
    torch.cuda.synchronize()
    x = xw[:, :cols].double()
    ref = x.sum(1) + (pre.double() if acc else 0.0)
    tol = (4 * -(-cols // 512) + 8) * U32 * x.abs().sum(1) + (2 * U32 * pre.double().abs() if acc else 0.0)
    oc = out.cpu()
    _assert_within(oc[:rows], ref, tol, 'out')
    assert torch.isnan(oc[rows:]).all(), 'out written beyond rows'


# ======================================================================================================================================
# 7. sf_cast_bf16
# ======================================================================================================================================
def _tie_heavy_matrix(rows, cols, g):
    """fp32 values of which a third are exact bf16 ties (low half = 0x8000, both parities of the kept mantissa LSB), a few are just above / below a tie,
    a few are fp32 subnormals and a few overflow bf16 under RNE; the rest random."""
    base = (torch.randn(rows, cols, generator=g) * 4.0).bfloat16().float().view(torch.int32)
    kind = torch.randint(0, 9, (rows, cols), generator=g)
    bits = base.clone()
    bits = torch.where(kind <= 2, base | 0x8000, bits)                      # exact ties
    bits = torch.where(kind == 3, base | 0x8001, bits)                      # just above a tie
    bits = torch.where(kind == 4, base | 0x7FFF, bits)                      # just below a tie
    bits = torch.where(kind == 5, torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, cols), generator=g, dtype=torch.int64).to(torch.int32), bits)
    x = bits.view(torch.float32)
    x = torch.where(torch.isfinite(x), x, torch.zeros(()))
    x[0, :4] = torch.tensor([3.4028235e38, -3.3961e38, 1e-40, -2.5e-39])    # rounds to inf; a tie-neighbourhood maximum; subnormals
    return x


@pytest.mark.parametrize('scale', [1.0, 0.75, float(np.float32(0.3))])
def test_cast_bf16_bit_exact(gpu, scale):
    """sf_cast_bf16: y = bf16(scale * x) is one fp32 multiply and one RNE rounding - bit-exact against torch fp32 + .bfloat16(), on a matrix dense in
    exact ties (both parities), near-ties, random bit patterns, subnormals and an overflowing value.  x and y are strided slices; y's canary columns and
    rows survive."""
    lib = _lib()
    dev = gpu
    rows, cols = 333, 772
    g = _gen(int(scale * 100))
    x = _tie_heavy_matrix(rows, cols, g)
    ldx, ldy = cols + 8, cols + 12
    xw = torch.full((rows, ldx), float('nan'))
    xw[:, 4:4 + cols] = x
    yw = torch.full((rows + 2, ldy), 7.0, dtype=torch.bfloat16, device=dev)
    xd = xw.to(dev)
    _ok(lib.sf_cast_bf16(xd[:, 4:].data_ptr(), ldx, yw[:, 4:].data_ptr(), ldy, rows, cols, scale, _st()), 'sf_cast_bf16')
    torch.cuda.synchronize()
    want = (x * torch.tensor(scale, dtype=torch.float32)).bfloat16()
    yg = yw.cpu()
    _assert_bits(yg[:rows, 4:4 + cols], want, 'y')
    assert (yg[:rows, :4].float() == 7.0).all() and (yg[:rows, 4 + cols:].float() == 7.0).all() and (yg[rows:].float() == 7.0).all(), 'canary'


# ======================================================================================================================================
# 8. sf_transpose_bf16 / sf_transpose_bf16_multi
# ======================================================================================================================================
def _rand_bits(shape, g):
    return torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


TRANSPOSE_CASES = [
    # R, C, R_pad, ld_in, ld_out, batch_outer, batch_inner, path
    (100, 136, 128, 144, 136, 2, 3, 'wide'),     # R, C not multiples of 64; zero fill 100..127
    (64, 64, 64, 64, 72, 1, 1, 'wide'),
    (77, 45, 96, 48, 104, 2, 2, 'narrow'),       # odd C forces the 32 x 32 kernel
    (70, 64, 80, 70, 88, 3, 1, 'narrow'),        # a row stride that is not a multiple of 8 forces it too
    (33, 40, 72, 40, 72, 1, 2, 'narrow'),        # everything wide-shaped but the batch strides (odd, below) -> 32 x 32
]


@pytest.mark.parametrize('R,C,R_pad,ld_in,ld_out,bo,bi,path', TRANSPOSE_CASES, ids=[f'{c[0]}x{c[1]}p{c[2]}-b{c[5]}x{c[6]}-{c[7]}' for c in TRANSPOSE_CASES])
def test_transpose_bf16_exact(gpu, R, C, R_pad, ld_in, ld_out, bo, bi, path):
    """sf_transpose_bf16: out[b0][b1][c][r] = in[b0][b1][r][c] for r < R, 0 for R <= r < R_pad - a move, so bit-exact on random bit patterns (NaN payloads
    included); both batch levels with distinct strides that leave gaps between the matrices; the wide 64 x 64 path and the 32 x 32 path (odd C, a row
    stride or batch stride that is not a multiple of 8).  Everything the kernel must not write (columns beyond R_pad, the gaps) keeps its canary."""
    dev = gpu
    g = _gen(R * C + bo)
    sI1 = R * ld_in + (8 if path == 'wide' else 3)
    sI0 = bi * sI1 + 16
    sO1 = C * ld_out + 8
    sO0 = bi * sO1 + 24
    if path == 'wide':
        assert C % 8 == 0 and R_pad % 8 == 0 and ld_in % 8 == 0 and ld_out % 8 == 0
    inp = _rand_bits((bo * sI0 + 8,), g)
    out = torch.full((bo * sO0 + 8,), 7.0, dtype=torch.bfloat16)
    ind, outd = inp.to(dev), out.to(dev)
    from synchformer_amd import train as T
    T.transpose(ind, ld_in, sI0, sI1, outd, ld_out, sO0, sO1, R, C, R_pad, bo, bi)
    torch.cuda.synchronize()
    want = out.view(torch.int16).clone()
    src = inp.view(torch.int16)
    for b0 in range(bo):
        for b1 in range(bi):
            a = src[b0 * sI0 + b1 * sI1:][:R * ld_in].reshape(R, ld_in)[:, :C]
            o = want[b0 * sO0 + b1 * sO1:][:C * ld_out].view(C, ld_out)
            o[:, :R] = a.t()
            o[:, R:R_pad] = 0
    assert torch.equal(outd.cpu().view(torch.int16), want), 'transpose differs (or wrote outside its rows / padding)'


def test_transpose_bf16_multi_matches_single_and_reference(gpu):
    """sf_transpose_bf16_multi over a hand-built device table of five tensors of different shapes (N % 64 != 0 with zero padding, one tile, a wide one, an
    output row stride beyond R_pad): bit-identical to per-tensor sf_transpose_bf16 and to w.t() with zero padding; canaries beyond R_pad survive."""
    from synchformer_amd import train as T
    lib = _lib()
    dev = gpu
    g = _gen(11)
    shapes = [(768, 768, 768), (100, 256, 256), (3072, 64, 64), (200, 136, 144), (64, 8, 8)]     # (N, K, row stride of w)
    ws, outs, singles, rows, prefix = [], [], [], [], [0]
    for i, (N, K, ldw) in enumerate(shapes):
        w = _rand_bits((N, ldw), g).to(dev)
        n_pad = -(-N // 64) * 64
        ld_out = n_pad + (16 if i == 1 else 0)
        o = torch.full((K, ld_out), 7.0, dtype=torch.bfloat16, device=dev)
        s = torch.full((K, ld_out), 7.0, dtype=torch.bfloat16, device=dev)
        tx, ty = n_pad // 64, -(-K // 64)
        rows.append([w.data_ptr(), o.data_ptr(), ldw, ld_out, N, K, n_pad, tx])
        prefix.append(prefix[-1] + tx * ty)
        ws.append(w), outs.append(o), singles.append(s)
        T.transpose(w, ldw, 0, 0, s, ld_out, 0, 0, N, K, n_pad)
    tab = torch.tensor(rows, dtype=torch.int64, device=dev)
    pre = torch.tensor(prefix, dtype=torch.int32, device=dev)
    _ok(lib.sf_transpose_bf16_multi(tab.data_ptr(), pre.data_ptr(), len(shapes), prefix[-1], _st()), 'sf_transpose_bf16_multi')
    torch.cuda.synchronize()
    for (N, K, ldw), w, o, s in zip(shapes, ws, outs, singles):
        n_pad = -(-N // 64) * 64
        want = torch.full(tuple(o.shape), 7.0, dtype=torch.bfloat16).view(torch.int16)
        want[:, :N] = w.cpu().view(torch.int16)[:, :K].t()
        want[:, N:n_pad] = 0
        assert torch.equal(o.cpu().view(torch.int16), s.cpu().view(torch.int16)), f'{N}x{K}: multi differs from single'
        assert torch.equal(o.cpu().view(torch.int16), want), f'{N}x{K}: differs from w.t() with zero padding'


# ======================================================================================================================================
# 9. sf_grad_norm
# ======================================================================================================================================
GRAD_NORM_CASES = [(n, off) for n in (0, 1, 3, 1023, 256 * 1024 + 5) for off in (0, 1)] + [(2 ** 26 + 3, 0)]


@pytest.mark.parametrize('n,offset', GRAD_NORM_CASES, ids=[f'{n}-{"unaligned" if o else "aligned"}' for n, o in GRAD_NORM_CASES])
def test_grad_norm_vs_fp64(gpu, n, offset):
    """sf_grad_norm: ||g||_2 of a flat fp32 buffer against fp64.  All terms are positive, so the sum's relative error is bounded by its depth: per thread
    ceil(n / 2^18) + 2 terms (the 16-byte loop and the tail), 2 + 6 + 2 levels of stage 1, ceil(1024 / 256) + 2 + 6 + 2 of stage 2, + 1 rounding per square:
    d = ceil(n / 2^18) + 28; the norm's relative error <= (d / 2) u + u (sqrt).  offset 1 shifts the buffer by one float: the unaligned scalar path.  The
    kernel promises a fixed summation order: three runs are bit-identical."""
    lib = _lib()
    dev = gpu
    gen = torch.Generator(device=dev).manual_seed(n + offset)
    buf = torch.randn(n + offset + 4, generator=gen, device=dev) * 1e-2
    buf[n + offset:] = 1e6                                          # beyond the end: would dominate the norm if read
    gv = buf[offset:]
    ws = torch.empty(1024, device=dev)
    outs = []
    for _ in range(3):
        o = torch.full((2,), float('nan'), device=dev)
        _ok(lib.sf_grad_norm(gv.data_ptr(), n, o.data_ptr(), ws.data_ptr(), _st()), 'sf_grad_norm')
        outs.append(o)
    torch.cuda.synchronize()
    ref = math.sqrt(float((gv[:n].cpu().double() ** 2).sum())) if n else 0.0
    got = outs[0][0].item()
    d = -(-n // 2 ** 18) + 28
    assert abs(got - ref) <= (0.5 * d + 1) * U32 * ref, f'norm {got!r} vs fp64 {ref!r}'
    assert math.isnan(outs[0][1].item()), 'norm_out[1] was written'
    for o in outs[1:]:
        _assert_bits(o[:1], outs[0][:1], 'repeated grad norm')

# ======================================================================================================================================
# 10. sf_dropout
# ======================================================================================================================================
def _keep_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))      # what the launcher computes on the host, in fp32


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_mask_is_a_function_of_seed_and_shape(gpu, p):
    """sf_dropout: the mask depends on (seed, rows, cols) only - the same for fp32 and bf16, contiguous and strided (row strides > cols, different on each
    side), out of place and in place; kept elements are exactly x * fp32(1 / (1 - p)) (one fp32 multiply: bit-exact, and for p = 0.5 exactly x / (1 - p)),
    dropped ones +0; bf16 output = RNE of that product.  With an fp32 residual: dropped elements are the residual bit for bit, kept ones within
    u |x ks| + u |y| (product and sum, possibly contracted).  Canary columns of the strided outputs survive."""
    from synchformer_amd import train as T
    dev = gpu
    rows, cols, seed = 300, 770, 0xC0FFEE
    g = _gen(int(p * 10))
    x = (torch.rand(rows, cols, generator=g) + 0.5) * torch.where(torch.rand(rows, cols, generator=g) < 0.5, -1.0, 1.0)
    ks = torch.tensor(_keep_scale(p))

    def run(xin, y, residual=None):
        T.dropout(xin, y, rows, cols, p, seed, residual=residual)
        torch.cuda.synchronize()
        return y[:, :cols].cpu()
    y32 = run(x.to(dev), torch.empty(rows, cols, device=dev))
    mask = y32 != 0
    _assert_bits(y32, torch.where(mask, x * ks, torch.zeros(())), 'fp32 kept values')
    if p == 0.5:
        assert torch.equal(y32[mask].double(), x[mask].double() / (1 - p))
    xw = torch.full((rows, cols + 6), float('nan'), device=dev)
    xw[:, :cols] = x.to(dev)
    yw = torch.full((rows, cols + 10), float('nan'), device=dev)
    ys = run(xw[:, :cols], yw[:, :cols])
    _assert_bits(ys, y32, 'fp32 strided')
    assert torch.isnan(yw[:, cols:]).all(), 'strided fp32 output written beyond cols'
    xi = x.to(dev).clone()
    _assert_bits(run(xi, xi), y32, 'fp32 in place')
    xb = x.bfloat16()
    yb = run(xb.to(dev), torch.empty(rows, cols, device=dev, dtype=torch.bfloat16))
    assert torch.equal(yb != 0, mask), 'bf16 mask differs from the fp32 mask'
    _assert_bits(yb, torch.where(mask, xb.float() * ks, torch.zeros(())).bfloat16(), 'bf16 kept values')
    xbw = torch.full((rows, cols + 14), 7.0, device=dev, dtype=torch.bfloat16)
    xbw[:, :cols] = xb.to(dev)
    ybw = torch.full((rows, cols + 2), 7.0, device=dev, dtype=torch.bfloat16)
    _assert_bits(run(xbw[:, :cols], ybw[:, :cols]), yb, 'bf16 strided')
    assert (ybw[:, cols:].float() == 7.0).all(), 'strided bf16 output written beyond cols'
    _assert_bits(run(xbw[:, :cols], xbw[:, :cols]), yb, 'bf16 in place')
    r = torch.randn(rows, cols, generator=g)
    rw = torch.full((rows, cols + 4), float('nan'), device=dev)
    rw[:, :cols] = r.to(dev)
    yr = run(x.to(dev), torch.empty(rows, cols, device=dev), residual=rw[:, :cols])
    assert torch.equal(yr[~mask], r[~mask]), 'dropped elements must be the residual'
    kept = (x * ks).double()
    ref = torch.where(mask, kept, torch.zeros((), dtype=torch.float64)) + r.double()
    _assert_within(yr[mask], ref[mask], (U32 * kept.abs() + U32 * ref.abs())[mask], 'kept + residual')


def test_dropout_p0_is_identity(gpu):
    """p = 0: every element kept with scale 1 - y is x bit for bit, fp32 and bf16 (random bit patterns, finite)."""
    from synchformer_amd import train as T
    dev = gpu
    g = _gen(3)
    x = torch.randn(129, 333, generator=g) * 100
    y = torch.empty_like(x, device=dev)
    T.dropout(x.to(dev), y, 129, 333, 0.0, 77)
    xb = x.bfloat16()
    yb = torch.empty_like(xb, device=dev)
    T.dropout(xb.to(dev), yb, 129, 333, 0.0, 77)
    torch.cuda.synchronize()
    _assert_bits(y, x, 'fp32 p=0')
    _assert_bits(yb, xb, 'bf16 p=0')


@pytest.mark.parametrize('p', [0.1, 0.25, 0.5])
def test_dropout_keep_rate_statistics(gpu, p):
    """Keep rate of sf_dropout over a matrix of ones (how DropPath and token dropout use it) within 5 sigma of 1 - p: overall, per row, per column, per
    column residue class (c mod k) and per linear-index residue class (i mod 2^j, i = r * cols + c - what the hash sees) - a hash that correlates with
    the index fails one of these.  Different seeds (neighbouring, and differing in the top bit only) give different masks that agree at the rate of two
    independent ones, p^2 + (1 - p)^2, within 5 sigma."""
    from synchformer_amd import train as T
    dev = gpu
    rows, cols = 2048, 1000
    ones = torch.ones(rows, cols, device=dev)

    def mask(seed):
        y = torch.empty(rows, cols, device=dev)
        T.dropout(ones, y, rows, cols, p, seed)
        torch.cuda.synchronize()
        return (y != 0).cpu()
    m = mask(12345)
    q = 1.0 - p

    def check(keep_frac, counts, what):
        sig = np.sqrt(p * q / counts)
        z = np.abs(keep_frac - q) / sig
        assert z.max() <= 5.0, f'{what}: keep rate {keep_frac.flat[z.argmax()]:.4f} vs {q} ({z.max():.1f} sigma)'
    mf = m.double().numpy()
    check(np.array([mf.mean()]), mf.size, 'overall')
    check(mf.mean(1), cols, 'per row')
    check(mf.mean(0), rows, 'per column')
    for k in (2, 3, 4, 5, 8, 16, 32, 64):
        cls = np.arange(cols) % k
        for j in range(k):
            sel = mf[:, cls == j]
            check(np.array([sel.mean()]), sel.size, f'columns = {j} mod {k}')
    flat = mf.reshape(-1)
    for jb in range(1, 11):
        k = 2 ** jb
        fr = flat.reshape(-1, k).mean(0)
        check(fr, flat.size // k, f'linear index mod {k}')
    for other in (12346, 12345 ^ 0x80000000):
        m2 = mask(other)
        assert not torch.equal(m, m2), f'seed {other} gave the same mask'
        agree = (m == m2).double().mean().item()
        pa = p * p + q * q
        assert abs(agree - pa) <= 5 * np.sqrt(pa * (1 - pa) / m.numel()), f'seed {other}: masks agree on {agree:.4f}, independent ones on {pa:.4f}'


# ======================================================================================================================================
# 11. GELU over every finite bf16 value: sf_gelu_fwd, sf_gelu_bwd, sf_gelu_bwd_bf16 and the GEMM GELU epilogues
# ======================================================================================================================================
EPS_ERF = 3e-7          # Abramowitz-Stegun 7.1.28: |erf(z) - (1 - t(z)^-16)| <= 3e-7 for z >= 0
# fp32 evaluation of r = 1 / t^16 (sf_common.h gelu_erf2 / gelu_erf4): Horner over six positive terms <= 12 u relative on t, ^16 by four squarings
# -> 16 * 12 u + 15 u, rcpf (v_rcp_f32) <= 2 u more: 210 u relative on r
R_REL = 210 * U32


def _bf16_sweep():
    """Every finite bf16 value (65,280 of them, +-0 and the subnormals included), in bit order."""
    b = torch.arange(65536, dtype=torch.int32)
    b = b[((b >> 7) & 0xFF) != 0xFF]
    return torch.where(b >= 32768, b - 65536, b).to(torch.int16).view(torch.bfloat16)


def _gelu_ref(x):
    x = x.double()
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def _gelu_fwd_bar(x):
    """1 bf16 ulp of the fp64 value + what the erf approximation allows: gelu = max(x, 0) - 0.5 |x| r with r ~ erfc(|x| / sqrt 2), so
    0.5 |x| (EPS_ERF + R_REL (erfc + EPS_ERF)) absolute."""
    x = x.double()
    ref = _gelu_ref(x)
    return _bf16_ulp(ref) + 0.5 * x.abs() * (EPS_ERF + R_REL * (torch.special.erfc(x.abs() / math.sqrt(2.0)) + EPS_ERF))


def _gelu_grad_ref(x):
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _gelu_bwd_bar(x, dact):
    """1 bf16 ulp of the fp64 value + |dact| * (the absolute error of Phi = fma(erff(x / sqrt 2), 0.5, 0.5): erff <= 2 ulp of |erf| < 1 (2^-23), halved, plus
    the argument's rounding and the fma's: <= 2^-23 in all; + the relative error of x * phi with phi from __expf(-0.5 x^2): the exponent's rounding is
    u * x^2 / 2 absolute, the scaling by log2 e another u * x^2 / 2, v_exp 1 ulp, the products 3 u -> (1.5 x^2 + 8) u * |x phi|)."""
    x, dact = x.double(), dact.double()
    ref = dact * _gelu_grad_ref(x)
    xphi = (x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)).abs()
    return ref, _bf16_ulp(ref) + dact.abs() * (2.0 ** -23 + (1.5 * x * x + 8) * U32 * xphi)


def _report_and_assert(name, x, got, ref, bar):
    """Prints the worst error relative to the bar (and where), per region, then asserts."""
    err = (got.double() - ref).abs()
    ratio = err / bar
    for label, sel in (('all', torch.ones_like(x, dtype=torch.bool)), ('x < -3', x.float() < -3), ('|x| < 2^-126', x.float().abs() < 2.0 ** -126)):
        if sel.any():
            r = ratio[sel]
            i = int(r.argmax())
            xs, es = x.float()[sel], err[sel]
            print(f'[gelu] {name:28s} {label:13s} max err/bar {r.max().item():.3g} at x = {xs[i].item():.6g} (err {es[i].item():.3g}, bar {bar[sel][i].item():.3g}); '
                  f'max |err| {es.max().item():.3g}')
    _assert_within(got, ref, bar, name)


def test_gelu_fwd_full_bf16_domain(gpu):
    """sf_gelu_fwd on all 65,280 finite bf16 inputs against fp64 x * Phi(x); bar _gelu_fwd_bar (1 bf16 ulp + the approximation's absolute allowance).
    Measured on MI355X: worst error 0.61 of the bar, at x = -3.859 (9.4e-7 against 1.5e-6); subnormal inputs within half an ulp."""
    lib = _lib()
    x = _bf16_sweep()
    n = x.numel()
    act = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=gpu)
    xd = x.to(gpu)
    _ok(lib.sf_gelu_fwd(xd.data_ptr(), act.data_ptr(), n, _st()), 'sf_gelu_fwd')
    torch.cuda.synchronize()
    a = act.cpu()
    assert (a[n:].float() == 7.0).all(), 'written beyond n'
    _report_and_assert('sf_gelu_fwd', x, a[:n], _gelu_ref(x), _gelu_fwd_bar(x))


@pytest.mark.parametrize('dact_kind', ['ones', 'random'])
def test_gelu_bwd_full_bf16_domain(gpu, dact_kind):
    """sf_gelu_bwd (fp32 dact) and sf_gelu_bwd_bf16 (bf16 dact) on all finite bf16 inputs against fp64 dact * (Phi(x) + x phi(x)); bar _gelu_bwd_bar.
    Measured on MI355X: worst error 0.50 of the bar (the final bf16 rounding), 0.49 of it for x < -3."""
    lib = _lib()
    x = _bf16_sweep()
    n = x.numel()
    g = _gen(9)
    dact = torch.ones(n) if dact_kind == 'ones' else torch.randn(n, generator=g) * 3
    xd = x.to(gpu)
    out = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=gpu)
    dad = dact.to(gpu)
    _ok(lib.sf_gelu_bwd(xd.data_ptr(), dad.data_ptr(), out.data_ptr(), n, _st()), 'sf_gelu_bwd')
    dab = dact.bfloat16()
    outb = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=gpu)
    dabd = dab.to(gpu)
    _ok(lib.sf_gelu_bwd_bf16(xd.data_ptr(), dabd.data_ptr(), outb.data_ptr(), n, _st()), 'sf_gelu_bwd_bf16')
    torch.cuda.synchronize()
    o, ob = out.cpu(), outb.cpu()
    assert (o[n:].float() == 7.0).all() and (ob[n:].float() == 7.0).all(), 'written beyond n'
    ref, bar = _gelu_bwd_bar(x, dact)
    _report_and_assert(f'sf_gelu_bwd dact={dact_kind}', x, o[:n], ref, bar)
    ref, bar = _gelu_bwd_bar(x, dab.float())
    _report_and_assert(f'sf_gelu_bwd_bf16 dact={dact_kind}', x, ob[:n], ref, bar)


def _identity_gelu_operands(dev):
    """A = I (256 x 256) and W (256 x 256) holding the sweep (padded with its first 256 values): out = A W^T = W^T exactly in fp32 (x * 1 plus zeros), so
    out[m, n] = gelu(W[n, m]) up to the epilogue alone."""
    x = _bf16_sweep()
    w = torch.cat([x, x[:256]]).view(256, 256)
    return x, torch.eye(256).bfloat16().to(dev), w.to(dev)


@pytest.mark.parametrize('cfg', [-1, 0, 4, 7, 11], ids=['auto', 'cfg0', 'cfg4', 'cfg7', 'cfg11'])
def test_gemm_gelu_epilogue_full_bf16_domain(gpu, cfg):
    """The GELU epilogue of every product configuration of sf_gemm_bf16 (test_kernels_gpu.PRODUCT_CFGS) over all finite bf16 values, by the identity-operand
    trick: same bar as sf_gelu_fwd (the epilogue is the same gelu_erf helper on the same fp32 value)."""
    from synchformer_amd import ops
    lib = _lib()
    x, a, w = _identity_gelu_operands(gpu)
    out = torch.full((258, 256), 7.0, dtype=torch.bfloat16, device=gpu)
    lib.sf_gemm_force_config(cfg)
    try:
        ops.gemm(a, w, None, out, M=256, gelu=True)
    finally:
        lib.sf_gemm_force_config(-1)
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[256:].float() == 7.0).all(), 'rows beyond M were written'
    got = o[:256].t().reshape(-1)[:x.numel()]
    _report_and_assert(f'sf_gemm_bf16 cfg {cfg}', x, got, _gelu_ref(x), _gelu_fwd_bar(x))


def test_gemm_gelu_dual_full_bf16_domain(gpu):
    """sf_gemm_bf16_gelu_dual over the same sweep: the pre-activation is the sweep itself bit for bit (W^T + zero bias), the activation within the
    sf_gelu_fwd bar."""
    lib = _lib()
    x, a, w = _identity_gelu_operands(gpu)
    bias = torch.zeros(256, device=gpu)
    pre = torch.full((258, 256), 7.0, dtype=torch.bfloat16, device=gpu)
    act = torch.full((258, 256), 7.0, dtype=torch.bfloat16, device=gpu)
    _ok(lib.sf_gemm_bf16_gelu_dual(a.data_ptr(), 256, w.data_ptr(), 256, bias.data_ptr(), pre.data_ptr(), act.data_ptr(), 256, 256, 256, 256, _st()),
        'sf_gemm_bf16_gelu_dual')
    torch.cuda.synchronize()
    p, ac = pre.cpu(), act.cpu()
    assert (p[256:].float() == 7.0).all() and (ac[256:].float() == 7.0).all(), 'rows beyond M were written'
    wt = w.cpu().t()
    # +0 + (-0) bias: the pre-activation of -0 is +0; every other value passes through unchanged
    want = torch.where(wt.float() == 0, torch.zeros((), dtype=torch.bfloat16), wt)
    _assert_bits(torch.where(p[:256].float() == 0, torch.zeros((), dtype=torch.bfloat16), p[:256]), want, 'pre-activation')
    got = ac[:256].t().reshape(-1)[:x.numel()]
    _report_and_assert('sf_gemm_bf16_gelu_dual', x, got, _gelu_ref(x), _gelu_fwd_bar(x))
