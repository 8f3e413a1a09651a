"""Host-side oracle of the GEMM tests (tests/test_gemm_gpu.py, tests/test_gemm_oracle_cpu.py): operand families, the float64 reference, an fp32
emulation of a correct kernel, the derived error bars and the two acceptance criteria.  Nothing here touches a GPU API: every function works on the
device its tensors live on, so the big tile-walk cases may run it on the device while everything else stays on the host.

The operation is   out = act(A W^T + bias) + R   with A (M, K) and W (N, K) in bf16 (or dequantised MXFP8), fp32 accumulation, act = identity or exact-erf
GELU, R an fp32 residual, out fp32 or bf16 (round-to-nearest-even).

Operand families
  exact  integer-valued operands (A in [-4, 4], W in [-8, 8], integer bias / residual): every partial sum is an integer below 2^24 for K <= 3072, so the fp32
         result does not depend on the summation order, the tiling or a k rotation - outputs are compared BIT FOR BIT with the int64 result.
  sparse the raw material of the fused qkv tests (tests/qkv_fused_oracle.py, which adds the powers of two and the marks): A rows with at most 16 entries +-1 at random
         columns, W integers in [-8, 8], bias integers in [-64, 64] (MXFP8: at most 12 bytes +-1 per row of A, W bytes 0 / +-1, scale bytes 126 .. 128), so that
         every sum stays below 2^8 units and is a bf16 number.
  wide   Gaussian operands whose magnitude changes per 32-deep k-block and per row (factors 2^-6 .. 2^5 on A, 2^-4 .. 2^3 on W, sigma 0.05), Gaussian
         bias, residual of sigma 2 plus an offset.  Two criteria, both against float64 computed from the very values the kernel reads:
           elementwise  |got - ref| <= MARGIN * (u_out |ref| + F),  F = (d + c) 2^-24 S,  S = sum_k |a_k w_k| + |bias| + |residual|,
                        u_out = 2^-8 for a bf16 output (0 for fp32: that rounding is the last addition's, counted in c), d the longest chain of dependent
                        fp32 additions behind one output (MFMA steps along k + the depth of one MFMA), c the additions of the epilogue;
           statistical  per 64 x 64 block of the output  ||got - ref||_2 <= STAT_FACTOR * ||emu - ref||_2 + ||F||_2, where emu accumulates the 32-deep
                        k-blocks one after another in fp32 and rounds where the kernel rounds.  The yardstick is the emulation's own distance from float64.
GELU: with x the pre-activation and Fx its fp32 term, F = (|gelu'(x)| + Fx) Fx (first order + the second-order remainder, |gelu''| <= 1.13 < 2)
      + 0.5 |x| (EPS_ERF + R_REL (erfc(|x| / sqrt 2) + EPS_ERF))   (the erf approximation, as _gelu_fwd_bar of tests/test_train_rowops_gpu.py)
      + 2 * 2^-24 |x|  (the product and the subtraction of max(x, 0) - 0.5 |x| r)  + 2^-24 (|gelu(x)| + |R|)  (the residual addition).
LayerNorm(768) of a row x with fp32 error ex per element: y = (x - mean) rstd gamma + beta,
      bar_y = bf16 ulp(y) + 64 * 2^-24 (|xhat gamma| + |beta| + |gamma| rstd mean|x|) + |gamma| rstd (ex + mean(ex) + |xhat| mean(|xhat| ex));
      the first two terms are the bar of test_add_scale_ln768_vs_fp64, the third of them is the mean's own rounding (2^-24 |mean| / std: what a row with a
      large common offset adds), the last one is the row's X error carried through the normalisation."""
import math

import torch

U32 = 2.0 ** -24            # fp32 unit roundoff
U_BF16 = 2.0 ** -8          # bf16: round-to-nearest moves a value by at most half an ulp <= 2^-8 |ref|
MARGIN = 1.5
STAT_FACTOR = 2.0
EPS_ERF = 3e-7              # Abramowitz-Stegun 7.1.28, the kernels' erf
R_REL = 210 * U32           # fp32 evaluation of 1 / t^16 (see tests/test_train_rowops_gpu.py)
C_EPI = 2                   # (acc + bias) + residual


def gen(seed):
    return torch.Generator().manual_seed(seed)


def depth(K, mfma):
    """Longest chain of dependent fp32 additions behind one accumulator: one MFMA per `kstep` of k, each summing `kstep` products.
    '16x16x32' v_mfma_f32_16x16x32_bf16 (gemm_bf16_kernel: configs 0 - 6, 8, 9, the batched GEMM), '32x32x16' v_mfma_f32_32x32x16_bf16 (persistent / quadrant-phased
    kernels: configs 7, 10, 11, 12, the dual kernel, sf_gemm_res_ln768), '32x32x64' v_mfma_scale_f32_32x32x64_f8f6f4 (the MXFP8 kernels)."""
    kstep = {'16x16x32': 32, '32x32x16': 16, '32x32x64': 64}[mfma]
    return K // kstep + kstep


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operand families
# ---------------------------------------------------------------------------------------------------------------------------------------------
def operands(family, M, N, K, seed, a_rows=None):
    """dict(a (a_rows >= M, K) bf16 - rows beyond M are NaN -, w (N, K) bf16, bias (N,) fp32, res (M, N) fp32) of one family."""
    g = gen(seed)
    a_rows = M + 3 if a_rows is None else a_rows
    if family == 'exact':
        a = torch.randint(-4, 5, (a_rows, K), generator=g).float()
        w = torch.randint(-8, 9, (N, K), generator=g).float()
        bias = torch.randint(-50, 51, (N,), generator=g).float()
        res = torch.randint(-2000, 2001, (M, N), generator=g).float()
    elif family == 'sparse':
        a = torch.zeros(a_rows, K).scatter_(1, torch.randint(0, K, (a_rows, 16), generator=g), torch.randint(0, 2, (a_rows, 16), generator=g).float() * 2 - 1)
        w = torch.randint(-8, 9, (N, K), generator=g).float()
        bias = torch.randint(-64, 65, (N,), generator=g).float()
        res = torch.zeros(M, N)
    elif family == 'wide':
        a = torch.randn(a_rows, K, generator=g) * torch.exp2(torch.randint(-6, 6, (a_rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
        w = torch.randn(N, K, generator=g) * 0.05 * torch.exp2(torch.randint(-4, 4, (N, K // 32), generator=g).float()).repeat_interleave(32, 1)
        bias = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g) * 2.0 + 0.5
    else:
        raise ValueError(family)
    a = a.bfloat16()
    a[M:] = float('nan')
    return dict(family=family, M=M, N=N, K=K, a=a, w=w.bfloat16(), bias=bias, res=res)


def mx_operands(family, M, N, K, seed):
    """MXFP8 operands built directly as bytes: aq (M, K) / wq (N, K) e4m3 bytes (never 0x7F / 0xFF) and per-32-block E8M0 scale bytes asc (M, K / 32),
    wsc (N, K / 32); exact: bytes encoding integers in [-4, 4] / [-8, 8] and scale bytes 126 .. 128 (every product a multiple of 2^-2, every partial sum below
    2^24 of them); sparse: at most 12 bytes +-1 per row of A, W bytes 0 / +-1, scale bytes 126 .. 128 (every sum at most 12 * 16 + 64 quarter units); wide: any finite byte, scale bytes 120 .. 134.  Plus bias / res as in operands()."""
    g = gen(seed)
    if family == 'exact':
        aq = torch.randint(-4, 5, (M, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
        wq = torch.randint(-8, 9, (N, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
        asc = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
        wsc = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
        bias = torch.randint(-50, 51, (N,), generator=g).float()
        res = torch.randint(-2000, 2001, (M, N), generator=g).float()
    elif family == 'sparse':
        aq = torch.zeros(M, K).scatter_(1, torch.randint(0, K, (M, 12), generator=g), torch.randint(0, 2, (M, 12), generator=g).float() * 2 - 1)
        aq = aq.to(torch.float8_e4m3fn).view(torch.uint8)
        wq = torch.randint(-1, 2, (N, K), generator=g).float().to(torch.float8_e4m3fn).view(torch.uint8)
        asc = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
        wsc = torch.randint(126, 129, (N, K // 32), generator=g).to(torch.uint8)
        bias = torch.randint(-64, 65, (N,), generator=g).float()
        res = torch.zeros(M, N)
    else:
        assert family == 'wide', family
        def bytes_(r):
            b = torch.randint(0, 256, (r, K), generator=g)
            b = torch.where((b & 0x7F) == 0x7F, b - 0x40, b)            # 0x7F / 0xFF (NaN) -> 0x3F / 0xBF
            return b.to(torch.uint8)
        aq, wq = bytes_(M), bytes_(N) & 0xBF                            # |w| < 2 (exponent field <= 7) and scales <= 2^-4: outputs of a few hundred at most,
        asc = torch.randint(120, 135, (M, K // 32), generator=g).to(torch.uint8)     # so that bias and residual stay visible next to the product
        wsc = torch.randint(120, 124, (N, K // 32), generator=g).to(torch.uint8)
        bias = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g) * 2.0 + 0.5
    return dict(family=family, M=M, N=N, K=K, aq=aq, asc=asc, wq=wq, wsc=wsc, a=mx_dequant(aq, asc), w=mx_dequant(wq, wsc), bias=bias, res=res)


def mx_dequant(q, sc):
    """e4m3 bytes (rows, K) and scale bytes (rows, K / 32) -> float64 values."""
    return q.view(torch.float8_e4m3fn).float().double() * torch.exp2(sc.double() - 127.0).repeat_interleave(32, 1)


def mx_planes(sc, rows_alloc, fill=0x55):
    """(rows, K / 32) scale bytes -> the stage-major planes (K / 128, rows_alloc, 4) the kernels read; rows beyond `rows` hold `fill`."""
    rows, nb = sc.shape
    p = torch.full((nb // 4, rows_alloc, 4), fill, dtype=torch.uint8)
    p[:, :rows] = sc.view(rows, nb // 4, 4).permute(1, 0, 2)
    return p


def mx_unplane(p, rows):
    return p[:, :rows].permute(1, 0, 2).reshape(rows, -1)


def mx_quant_ref(x):
    """OCP MXFP8 quantisation of a bf16 matrix (the restatement of tests/test_kernels_gpu.py::_mx_quant_ref): scale 2^(floor(log2 amax) - 8) per 32-block,
    elements rounded to nearest-even e4m3 after saturation to +-448.  Returns bytes (R, K) and scale bytes (R, K / 32)."""
    xf = x.float()
    R, K = xf.shape
    blk = xf.view(R, K // 32, 32)
    amax = blk.abs().amax(-1)
    e = torch.floor(torch.log2(torch.clamp(amax, min=2.0 ** -126))) - 8
    byte = torch.clamp(e + 127, 1, 254)
    q = torch.clamp(blk * torch.exp2(127 - byte).unsqueeze(-1), -448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(R, K).view(torch.uint8), byte.to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference, fp32 emulation, bars
# ---------------------------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def reference(a, w, bias=None):
    """float64 pre-activation a w^T + bias and S = sum_k |a_k w_k| + |bias| from the (bf16 / dequantised) values the kernel reads."""
    ad, wd = a.double(), w.double()
    pre, S = ad @ wd.t(), ad.abs() @ wd.abs().t()
    if bias is not None:
        pre, S = pre + bias.double(), S + bias.double().abs()
    return pre, S


def mx_group_term(a, w, chunk=256):
    """The extra term of the MXFP8 kernels' bars (added AFTER the first measurement on the MI355X; see the module docstring of tests/test_gemm_gpu.py):
    v_mfma_scale_f32_32x32x64_f8f6f4 does not sum its products as an fp32 chain.  Probed through sf_gemm_mxfp8 with one large product p and smaller ones next to it:
    inside a group of 8 consecutive k every product is aligned to the group's largest and cut below 2^-13 of that one's power of two (p = 57344: 4 survives, 2 is
    lost, whatever else the group holds); across groups, 32-blocks and MFMA steps the sums behave like fp32.  So every product but the largest of its group may
    lose up to 2^-13 |p_max|:   7 * 2^-13 * sum over the groups g of 8 consecutive k of max_{k in g} |a_k w_k|   per output element (a, w: the dequantised values)."""
    a32, w32 = a.abs().float(), w.abs().float()
    M, K = a32.shape
    N = w32.shape[0]
    wg = w32.view(N, K // 8, 8)
    out = torch.empty(M, N, dtype=torch.float64, device=a.device)
    for r0 in range(0, M, chunk):
        ag = a32[r0:r0 + chunk].view(-1, K // 8, 8)
        acc = torch.zeros(ag.shape[0], N, dtype=torch.float32, device=a.device)
        for g in range(K // 8):
            acc += (ag[:, None, g, :] * wg[None, :, g, :]).amax(-1)
        out[r0:r0 + chunk] = acc
    return 7 * 2.0 ** -13 * out


def expected(pre, S, res, *, gelu, out_bf16, d, exact_pre=False, extra=None):
    """ref (float64), F (the fp32 term of the bar) and bar (elementwise) of out = act(pre) + res.  exact_pre: the pre-activation carries no rounding (family
    `exact`), so only the activation's and the residual addition's terms remain.  extra: a further term of the pre-activation's error (mx_group_term)."""
    r = res.double() if res is not None else None
    if not gelu:
        ref = pre if r is None else pre + r
        F = (d + C_EPI) * U32 * (S if r is None else S + r.abs())
        if exact_pre:
            F = torch.zeros_like(F)
        elif extra is not None:
            F = F + extra
    else:
        Fx = torch.zeros_like(S) if exact_pre else (d + 1) * U32 * S + (0.0 if extra is None else extra)
        g = gelu64(pre)
        x = pre.abs()
        F = (gelu_grad64(pre).abs() + Fx) * Fx + 0.5 * x * (EPS_ERF + R_REL * (torch.special.erfc(x / math.sqrt(2.0)) + EPS_ERF)) + 2 * U32 * x
        ref = g if r is None else g + r
        if r is not None:
            F = F + U32 * (g.abs() + r.abs())
    bar = MARGIN * ((U_BF16 * ref.abs() if out_bf16 else 0.0) + F)
    return dict(ref=ref, F=F, bar=bar)


def round_bf16(x, rtz=False):
    """fp32 -> bf16 (as fp32 values): round-to-nearest-even, or toward zero (the corruption)."""
    if not rtz:
        return x.bfloat16().float()
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(a, w, bias, res, *, gelu, out_bf16, kblock=32, kblocks=None, round_acc_after=None, rtz=False):
    """fp32 emulation of a correct kernel: the k-blocks accumulated one after another in fp32, then (acc + bias), GELU, + residual, the output rounded to
    bf16 where the kernel's is.  kblocks (the sequence of k-block indices to accumulate), round_acc_after (round the accumulator to bf16 after that many
    blocks) and rtz (output rounded toward zero) are the corruptions of tests/test_gemm_oracle_cpu.py."""
    af, wf = a.float(), w.float()
    K = af.shape[1]
    acc = torch.zeros(af.shape[0], wf.shape[0], dtype=torch.float32, device=af.device)
    for n, j in enumerate(range(K // kblock) if kblocks is None else kblocks):
        acc = acc + af[:, j * kblock:(j + 1) * kblock] @ wf[:, j * kblock:(j + 1) * kblock].t()
        if round_acc_after is not None and n + 1 == round_acc_after:
            acc = round_bf16(acc)
    if bias is not None:
        acc = acc + bias.float()
    if gelu:
        acc = torch.nn.functional.gelu(acc)
    if res is not None:
        acc = acc + res.float()
    return round_bf16(acc, rtz) if out_bf16 else acc


def layernorm64(x, gamma, beta, eps, ex=None):
    """float64 LayerNorm over 768 columns of x (rows, 768) and the elementwise bar of a bf16 output (see the module docstring); ex = the fp32 error bar of x."""
    x, g, b = x.double(), gamma.double(), beta.double()
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xh = xc * rstd
    y = xh * g + b
    F = 64 * U32 * ((xh * g).abs() + b.abs() + g.abs() * rstd * x.abs().mean(1, keepdim=True))
    if ex is not None:
        ex = ex.double()
        F = F + g.abs() * rstd * (ex + ex.mean(1, keepdim=True) + xh.abs() * (xh.abs() * ex).mean(1, keepdim=True))
    return y, bf16_ulp(y) + F


def bf16_ulp(ref):
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def exact_mismatch(got, ref, out_bf16):
    """Elements of `got` whose bits differ from the (integer-valued, float64 or int64) reference rounded once to the output type; None when all agree."""
    want = ref.float()
    if out_bf16:
        want = want.bfloat16()
        got = got.bfloat16()
    else:
        got = got.float()
    bad = bits(got) != bits(want)
    if not bad.any():
        return None
    i = bad.nonzero()[0].tolist()
    rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
    return (f'{int(bad.sum())} of {bad.numel()} elements differ bitwise (rows {int(rows[0])}..{int(rows[-1])}, {rows.numel()} of them; columns '
            f'{int(cols[0])}..{int(cols[-1])}, {cols.numel()} of them); first at {i}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}')


def wide_check(got, exp, emu, block=64):
    """Both criteria of the `wide` family.  Returns dict(elem = worst |err| / bar, stat = worst block ||got - ref|| / limit, msg = None or what failed)."""
    ref, bar, F = exp['ref'], exp['bar'], exp['F']
    err = (got.double() - ref).abs()
    bad = ~(err <= bar)                              # a NaN fails
    elem = float(torch.nan_to_num(err / bar.clamp_min(1e-300), nan=float('inf')).max())
    msgs = []
    if bad.any():
        i = bad.nonzero()[0].tolist()
        msgs.append(f'{int(bad.sum())} of {bad.numel()} elements outside the bar (worst err / bar {elem:.3g}); first at {i}: got {got[tuple(i)].item()!r} '
                    f'want {ref[tuple(i)].item()!r} bar {bar[tuple(i)].item()!r}')
    def block_norms(t):                              # (ceil(M / block), ceil(N / block)) l2 norms, the ragged edge blocks zero-padded
        M, N = t.shape
        t = torch.nn.functional.pad(t * t, (0, -N % block, 0, -M % block))
        return t.view(t.shape[0] // block, block, t.shape[1] // block, block).sum((1, 3)).sqrt()
    en = block_norms(torch.nan_to_num(err, nan=float('inf'), posinf=float('inf')))
    lim = STAT_FACTOR * block_norms(emu.double() - ref) + block_norms(F)
    ratio = torch.where(lim > 0, en / lim.clamp_min(1e-300), torch.where(en == 0, torch.zeros_like(en), torch.full_like(en, float('inf'))))
    stat = float(ratio.max())
    for i in (~(ratio <= 1.0)).nonzero()[:3].tolist():
        msgs.append(f'block rows {i[0] * block}.. columns {i[1] * block}..: ||got - ref|| = {float(en[tuple(i)]):.4g} > {STAT_FACTOR} * ||emu - ref|| + ||F|| = '
                    f'{float(lim[tuple(i)]):.4g}')
    return dict(elem=elem, stat=stat, msg='; '.join(msgs) if msgs else None)


def canary(shape, dtype):
    """A position-dependent prefill for an output buffer: NaNs whose payload is the element's index (fp32 / bf16), index-derived bytes (uint8)."""
    n = 1
    for s in shape:
        n *= s
    idx = torch.arange(n, dtype=torch.int64)
    if dtype == torch.float32:
        return (0x7FC00000 | (idx % 0x3FFFFF + 1)).to(torch.int32).view(torch.float32).reshape(shape)
    if dtype == torch.bfloat16:
        return (0x7F80 | (idx % 127 + 1)).to(torch.int16).view(torch.bfloat16).reshape(shape)
    if dtype == torch.uint8:
        return ((idx * 37 + 11) % 251).to(torch.uint8).reshape(shape)
    raise ValueError(dtype)


def canary_damage(got, prefill, written):
    """None when every element of `got` outside the boolean mask `written` still holds the prefill's bits, else a description."""
    bad = (bits(got) != bits(prefill)) & ~written
    if not bad.any():
        return None
    return f'{int(bad.sum())} elements outside the output were written, first at {bad.nonzero()[0].tolist()}'
