"""Host-side oracle of the forward row / gather / MXFP8 / mel tests (tests/test_rowops_fwd_gpu.py, tests/test_rowops_fwd_oracle_cpu.py): input families, float64 or
integer references of every operation, fp32 emulations of a correct kernel in the kernel's own order, the error bars and the emulated defects the criteria must
reject.  Nothing here touches a GPU API.  canary / canary_damage / layernorm64 / bf16_ulp / bits / mx_planes / mx_unplane are gemm_oracle's.

LayerNorm(768)   y = (x - mean) rstd gamma + beta per row; reference and bar = gemm_oracle.layernorm64 as it stands (bf16 ulp(y) + 64 * 2^-24 (|xhat gamma| + |beta|
                 + |gamma| rstd mean|x|)); an fp32 output drops the bf16-ulp term, accumulate adds 2^-24 (|prefill| + |y|).  Families: gauss, offset100 (100 +
                 N(0, 1): a one-pass variance loses three digits), offset1e4 (1e4 + 1e-2 N(0, 1)), spike (one 1e3 among 1e-3), scales (rows scaled 2^-20 .. 2^19),
                 const (constant integer rows: variance exactly 0, what remains is the mean's own rounding times rstd <= eps^-1/2 - the bar's third term).
MXFP8            scale byte = clamp(biased exponent of the block's largest magnitude - 8, 1, 254), element = RNE to e4m3 of x * 2^(127 - byte) saturated to +-448, sign
                 kept: integer arithmetic on the bf16 bit patterns (mx_quant_int); no log2, no float8 cast.  mx_blocks() pairs chosen block maxima with probes.
moves            bf16 = round-to-nearest-even of the fp32 bits (rne_bf16_bits), everything else bit for bit.
patch gathers    u8_table(): the 256 outputs of the u8 front-end written in numpy float16; video_patches / spec_patches: the index maps.
token masks      the literal rule: the indicator (1 kept, inf masked) dotted with filter 0 in float64 is NaN (token_keep_literal).
mel front-end    float64 from the very fp32 tables; the elementwise bar of mel_reference (worst case of the fp32 chains, written before the first run):
                   e_re = 401 * 2^-24 sum_m |x_m c_m| (400 fma + slack), e_im likewise;  e_P = 2 |re| e_re + 2 |im| e_im + e_re^2 + e_im^2 + 3 * 2^-24 P;
                   e_A = sum_k fb e_P + (n_k + 1) 2^-24 A  (n_k = the filter's bins);  e_v = the log of the relative change of A + 1e-6 (the addition's rounding
                   included; the computed sum is never below the floor itself, which bounds the downward change) + LOGF_ULP ulp of logf;
                   bar = e_v inv + 3 * 2^-24 |out|  (three roundings of (v - mean) * inv).
                 LOGF_ULP = 2: the ROCm device-library documentation is not installed next to the compiler here, so the figure asked for is the fallback of 2 ulp.
                 Bins that hold only leakage below the 1e-6 floor (tones, DC) make that bar vacuous; there the per-frame l2 criterion of mel_frame_check holds the
                 kernel to the fp32 emulation in its own order (sequential fma over m, then sequential fma over k in [fb_lo, fb_hi))."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402

U32 = G.U32
D = 768
INF = float('inf')
MEL_CAP = 5e-3               # the largest bar that still holds an element of the mel output
LOGF_ULP = 2.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------------
def elem_check(got, ref, bar):
    """Every element of got against ref +- bar (float64).  dict(worst = largest err / bar, msg = None or what failed); a NaN fails."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bar)
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
    worst = float(torch.nan_to_num(ratio, nan=INF).max()) if ratio.numel() else 0.0
    if not bad.any():
        return dict(worst=worst, msg=None)
    i = tuple(bad.nonzero()[0].tolist())
    return dict(worst=worst, msg=f'{int(bad.sum())} of {bad.numel()} elements outside the bar (worst err / bar {worst:.3g}); first at {list(i)}: got '
                                 f'{got[i].item()!r} want {ref[i].item()!r} bar {bar[i].item()!r}')


def bits_mismatch(got, want):
    """None when got and want (same shape and element size) agree bit for bit, else a description."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    bad = G.bits(got) != G.bits(want)
    if not bad.any():
        return None
    i = tuple(bad.nonzero()[0].tolist())
    return f'{int(bad.sum())} of {bad.numel()} elements differ bitwise, first at {list(i)}: got {int(G.bits(got)[i]) & 0xFFFFFFFF:#x} want {int(G.bits(want)[i]) & 0xFFFFFFFF:#x}'


def map_rows(m, rows):
    """Physical rows of the logical rows 0 .. rows - 1 under a 6-integer row map (None = identity)."""
    r = torch.arange(rows, dtype=torch.int64)
    if m is None:
        return r
    n12, n2, sA, s1, s2, off = m
    a, rem = r // n12, r % n12
    return a * sA + (rem // n2) * s1 + (rem % n2) * s2 + off


def drop_tail_rows(out, prefill, rows):
    """The defect 'rows beyond the last whole group of 4 are not processed': those rows of `out` keep the prefill."""
    bad = out.clone()
    keep = rows - rows % 4
    bad[keep:rows] = prefill[keep:rows]
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm(768)
# ---------------------------------------------------------------------------------------------------------------------------------------------
LN_FAMILIES = ('gauss', 'offset100', 'offset1e4', 'spike', 'scales', 'const')
LN_EPS = (1e-12, 1e-6, 1e-5)
_CONST = (5, -3, 0, 1, 100, -7, 12, 2, 33)


def ln_params(seed):
    g = G.gen(seed)
    return 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def ln_input(family, rows, seed):
    g = G.gen(seed)
    z = torch.randn(rows, D, generator=g)
    r = torch.arange(rows)
    if family == 'gauss':
        return 3.0 * z + 0.5
    if family == 'offset100':
        return 100.0 + z
    if family == 'offset1e4':
        return 1e4 + 1e-2 * z
    if family == 'spike':
        x = 1e-3 * z
        x[r, torch.randint(0, D, (rows,), generator=g)] = 1e3
        return x
    if family == 'scales':
        return z * torch.exp2(((r * 7 + seed) % 40 - 20).float()).unsqueeze(1)
    if family == 'const':
        return torch.tensor(_CONST, dtype=torch.float32)[(r + seed) % len(_CONST)].unsqueeze(1).expand(rows, D).contiguous()
    raise ValueError(family)


def ln_expected(x, gamma, beta, eps, out_bf16, prefill=None):
    """(ref, bar) float64 of y (= | +=) LayerNorm(x): layernorm64's bar, without its bf16-ulp term for an fp32 output, + 2^-24 (|prefill| + |y|) for accumulate."""
    y, bar = G.layernorm64(x, gamma, beta, eps)
    if not out_bf16:
        bar = (bar - G.bf16_ulp(y)).clamp_min(0.0)
    if prefill is not None:
        p = prefill.double()
        return p + y, bar + U32 * (p.abs() + y.abs())
    return y, bar


def _wave_sum(s):
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, :1]                                   # the butterfly leaves every lane with the same bits (fp32 addition commutes)


def ln_emulate(x, gamma, beta, eps, out_bf16=False, prefill=None, one_pass=False):
    """fp32 emulation of layernorm768_kernel's order: lane l of 64 holds columns i * 256 + 4 l .. + 3 (i < 3) and sums (a + b) + (c + d) per i, the lanes combine in
    an xor butterfly 32 .. 1, two passes (mean, then the centred squares).  one_pass: the defect var = E[x^2] - mean^2."""
    x = x.float()
    rows = x.shape[0]
    v = x.view(rows, 3, 64, 4)
    inv_d, eps32 = torch.tensor(1.0 / D, dtype=torch.float32), torch.tensor(eps, dtype=torch.float32)
    s = torch.zeros(rows, 64)
    for i in range(3):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mean = _wave_sum(s) * inv_d
    c = v - mean.view(rows, 1, 1, 1)
    sq = v if one_pass else c
    q = torch.zeros(rows, 64)
    for i in range(3):
        q = q + ((sq[:, i, :, 0] * sq[:, i, :, 0] + sq[:, i, :, 1] * sq[:, i, :, 1]) + (sq[:, i, :, 2] * sq[:, i, :, 2] + sq[:, i, :, 3] * sq[:, i, :, 3]))
    var = _wave_sum(q) * inv_d
    if one_pass:
        var = var - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps32)
    o = (c * rstd.view(rows, 1, 1, 1)).reshape(rows, D) * gamma.float() + beta.float()
    if prefill is not None:
        o = o + prefill.float()
    return o.bfloat16() if out_bf16 else o


# ---------------------------------------------------------------------------------------------------------------------------------------------
# MXFP8 quantisation, on bit patterns
# ---------------------------------------------------------------------------------------------------------------------------------------------
_BITLEN = torch.tensor([int(i).bit_length() for i in range(256)], dtype=torch.int64)


def bf16_fields(xb):
    """bf16 tensor -> (sign, M, E, mag) int64 with |x| = M * 2^E (M < 256) and mag = the 15 magnitude bits (monotone in |x|).  Finite inputs."""
    u = G.bits(xb).to(torch.int64) & 0xFFFF
    e, m = (u >> 7) & 0xFF, u & 0x7F
    return u >> 15, torch.where(e > 0, m + 128, m), e.clamp_min(1) - 134, u & 0x7FFF


def e4m3_bits(sign, M, s, truncate=False):
    """The e4m3 byte of (-1)^sign * M * 2^s (integers, 0 <= M < 256) rounded to nearest-even after saturation to 448.  e4m3: 3 mantissa bits, normals from 2^-6,
    subnormal step 2^-9; its codes are monotone in the magnitude, so code = ((max(p, -6) + 6) << 3) + n with p = floor(log2 v) and n = v in units of the binade's
    step 2^(max(p, -6) - 3) - a rounding carry (n = 16) lands on the next binade by itself.  truncate: the defect 'round toward zero'."""
    p = _BITLEN[M] - 1 + s
    pe = p.clamp_min(-6)
    r = pe - 3 - s                                    # v = (M / 2^r) steps
    Ms = M << (-r).clamp_min(0)
    rr = r.clamp(0, 40)                               # M < 2^8: a shift of 40 already gives 0 in either rounding
    half = (torch.ones_like(rr) << rr) >> 1
    n = Ms >> rr if truncate else torch.where(rr == 0, Ms, (Ms + half - 1 + ((Ms >> rr) & 1)) >> rr)
    code = torch.where(M == 0, torch.zeros_like(M), (((pe + 6) << 3) + n).clamp_max(0x7E))
    return code | (sign << 7)


def mx_quant_int(xb, rule=0, truncate=False):
    """sf_quantize_mxfp8 of a finite bf16 matrix (R, K), K % 32 == 0, in integer arithmetic -> (bytes (R, K) uint8, scale bytes (R, K / 32) uint8).
    rule 1: the round-up scale rule (one exponent up when the maximum's mantissa exceeds 1.75), the defect where rule 0 is expected."""
    R, K = xb.shape
    sign, M, E, mag = bf16_fields(xb)
    amax = mag.view(R, K // 32, 32).amax(-1)
    be = (amax >> 7) - 8
    if rule == 1:
        be = be + ((amax & 0x7F) > 0x60).to(torch.int64)
    byte = be.clamp(1, 254)
    q = e4m3_bits(sign, M, E + 127 - byte.repeat_interleave(32, 1), truncate)
    return q.to(torch.uint8), byte.to(torch.uint8)


MX_MAX_EXP = (1, 2, 119, 127, 135, 254, 0)            # biased: 2^-126, 2^-125, 2^-8, 2^0, 2^8, 2^127, bf16 subnormal
MX_MAX_MANT = (0x00, 0x60, 0x61, 0x7F)                # 1.0, 1.75, the bf16 just above 1.75, 1.9921875


def mx_blocks(seed=0):
    """Constructed 32-element blocks as bf16 bit patterns, (n_blocks, 32) int64.  A block's scale depends only on its maximum, so each block pairs one chosen
    maximum (MX_MAX_EXP x MX_MAX_MANT, either sign, at a moving position) with 31 probes: every 7-bit mantissa at 2^0 .. 2^-20 below the maximum's exponent
    (never above the maximum; what falls below 2^-126 becomes a bf16 subnormal), random signs - e4m3 ties, subnormals, underflow to +-0 and, above 1.75,
    saturating values.  Then a block of +-0 under each maximum class 2^0, and the all-zero blocks (+0; mixed +-0)."""
    g = G.gen(seed)
    t = torch.arange(21).repeat_interleave(128)
    m = torch.arange(128).repeat(21)
    out = []
    for e in MX_MAX_EXP:
        for ma in MX_MAX_MANT:
            ma = max(ma, 1) if e == 0 else ma
            top = (e << 7) | ma
            if e == 0:
                probes = (m % (ma + 1)) >> t
            else:
                mm = torch.where(t == 0, m % (ma + 1), m)
                ep = e - t
                probes = torch.where(ep >= 1, (ep.clamp_min(1) << 7) | mm, (128 + mm) >> (1 - ep).clamp(0, 40))
            probes = probes[torch.randperm(probes.numel(), generator=g)]
            probes = torch.cat([probes, probes[:(-probes.numel()) % 31]]).view(-1, 31)
            probes = probes | (torch.randint(0, 2, probes.shape, generator=g) << 15)
            blk = torch.empty(probes.shape[0], 32, dtype=torch.int64)
            pos = (torch.arange(probes.shape[0]) * 7 + len(out)) % 32
            cols = torch.arange(32).unsqueeze(0).expand_as(blk)
            blk[cols != pos.unsqueeze(1)] = probes.reshape(-1)
            blk[torch.arange(blk.shape[0]), pos] = top | (torch.randint(0, 2, (blk.shape[0],), generator=g) << 15)
            out.append(blk)
    zeros = torch.zeros(3, 32, dtype=torch.int64)
    zeros[0, 5] = 127 << 7                            # +-0 next to a maximum of 1.0
    zeros[0, 6::2] = 0x8000
    zeros[2, ::3] = 0x8000                            # an all-zero block of mixed signs (block 1: all +0)
    return torch.cat(out + [zeros])


def mx_matrix(blocks, rows, K, start=0):
    """(rows, K) bf16 filled with rows * K / 32 of the constructed blocks, taken cyclically from block `start`."""
    n = rows * (K // 32)
    idx = (start + torch.arange(n)) % blocks.shape[0]
    return blocks[idx].to(torch.int16).view(torch.bfloat16).reshape(rows, K)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# moves and casts
# ---------------------------------------------------------------------------------------------------------------------------------------------
def rne_bf16_bits(x):
    """fp32 tensor (no NaN) -> bf16 tensor, round-to-nearest-even on the bit pattern: (u + 0x7FFF + bit 16) >> 16."""
    u = G.bits(x.float()).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int16).view(torch.bfloat16)


def f32_probes(shape, seed):
    """fp32 values around the bf16 rounding: a random non-NaN upper half over a lower half drawn from {0x8000 (the tie), 0x7FFF, 0x8001 (one fp32 ulp to either side),
    0, random}; every 64th element +-inf, every 64th (offset 32) an fp32 subnormal."""
    g = G.gen(seed)
    n = 1
    for s in shape:
        n *= s
    hi = torch.randint(0, 1 << 16, (n,), generator=g)
    hi = torch.where(((hi >> 7) & 0xFF) == 0xFF, hi & 0xBFFF, hi)                 # exponent 255 -> 127: no NaN, no accidental inf
    lo = torch.tensor([0x8000, 0x7FFF, 0x8001, 0, -1])[torch.randint(0, 5, (n,), generator=g)]
    lo = torch.where(lo < 0, torch.randint(0, 1 << 16, (n,), generator=g), lo)
    u = (hi << 16) | lo
    i = torch.arange(n)
    u = torch.where(i % 64 == 0, 0x7F800000 | ((i // 64) % 2 << 31), u)           # +-inf
    u = torch.where(i % 64 == 32, (u & 0x807FFFFF) | (1 << 15), u)                # fp32 subnormals (exponent field 0)
    return torch.where(u >= 1 << 31, u - (1 << 32), u).to(torch.int32).view(torch.float32).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# patch gathers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def u8_table():
    """bf16 outputs (256,) of the u8 front-end (RGBToHalfToZeroOne + RGBNormalize(0.5, 0.5) on half tensors): f16(b / 255), f16(a - 0.5), * 2 (exact), RNE to bf16 -
    in numpy float16 arithmetic (each operation: exact result rounded once to fp16)."""
    b = np.arange(256).astype(np.float16)
    a = (b / np.float16(255)).astype(np.float16)
    c = (a - np.float16(0.5)).astype(np.float16)
    return rne_bf16_bits(torch.from_numpy((c * np.float16(2)).astype(np.float32)))


def video_input(dtype, shape, seed):
    """(vid of `dtype` and `shape`, want = the bf16 value every element must arrive as, same shape).  u8: random over all 256 bytes; f16: random finite patterns
    (subnormals, values on bf16 ties) with +-65504 and the extreme subnormals planted; bf16: random non-NaN patterns, pass through; f32: f32_probes without inf."""
    g = G.gen(seed)
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.uint8:
        vid = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
        want = u8_table()[vid.long()]
    elif dtype == torch.float16:
        u = torch.randint(0, 1 << 16, (n,), generator=g)
        u = torch.where(((u >> 10) & 0x1F) == 0x1F, u & 0xBFFF, u)                # finite
        u[:6] = torch.tensor([0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x0000])
        vid = u.to(torch.int16).view(torch.float16)
        want = rne_bf16_bits(vid.float())
    elif dtype == torch.bfloat16:
        u = torch.randint(0, 1 << 16, (n,), generator=g)
        u = torch.where((((u >> 7) & 0xFF) == 0xFF) & ((u & 0x7F) != 0), u & 0xFF80, u)   # NaN -> inf
        vid = u.to(torch.int16).view(torch.bfloat16)
        want = vid.clone()
    else:
        vid = f32_probes((n,), seed)
        vid = torch.where(torch.isinf(vid), torch.full_like(vid, 0.3330078125), vid)
        want = rne_bf16_bits(vid)
    return vid.reshape(shape), want.reshape(shape)


def video_patches(x):
    """(N, 16, 3, 224, 224) frame-major segments -> (N * 1568, 1536): row = n * 1568 + f * 196 + h * 14 + w, column = ((c * 2 + dt) * 16 + dh) * 16 + dw."""
    N = x.shape[0]
    return x.permute(0, 2, 1, 3, 4).reshape(N, 3, 8, 2, 14, 16, 14, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N * 1568, 1536)


def clip_segments(x, frame0, seg_stride, n_seg):
    """(n_clips, T, 3, 224, 224) -> (n_clips * n_seg, 16, 3, 224, 224): segment (clip, s) = frames [frame0 + s * seg_stride, + 16)."""
    return torch.stack([x[c, frame0 + s * seg_stride: frame0 + s * seg_stride + 16] for c in range(x.shape[0]) for s in range(n_seg)])


def spec_patches(spec):
    """(N, F, Ta) -> (N * nf * nt, 256): Conv2d(k 16, stride 10) patches, row = (n * nf + fi) * nt + ti, column = df * 16 + dt."""
    p = spec.unfold(1, 16, 10).unfold(2, 16, 10)
    return p.reshape(-1, 256)


def swap_patch_rows(p, a=3, b=4):
    """The defect 'two patch-rows swapped': columns of dh = a and dh = b exchanged in every (c, dt) plane of a (rows, 1536) gather."""
    q = p.clone().view(p.shape[0], -1, 16, 16)
    q[:, :, a], q[:, :, b] = p.view(p.shape[0], -1, 16, 16)[:, :, b], p.view(p.shape[0], -1, 16, 16)[:, :, a]
    return q.view(p.shape)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# token masks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def token_keep_literal(patches_keep, w0):
    """The reference's rule, literally: the indicator (1 = kept, inf = masked content) of every patch (.., K) dotted with filter 0 (K,) in float64; the token is
    masked iff the result is NaN (inf * 0, or inf - inf).  -> bool (..), True = keep."""
    ind = torch.where(patches_keep, 1.0, INF).double()
    return ~torch.isnan((ind * w0.double()).sum(-1))


def token_keep_no_zero(patches_keep, w0):
    """The defect 'a zero weight under a masked pixel is ignored': only weights of both signs mask a token."""
    m = ~patches_keep
    return ~((m & (w0 > 0)).any(-1) & (m & (w0 < 0)).any(-1))


V_PLUS, V_MINUS, V_ZERO = ((0, 0), (64, 15), (63, 0)), ((63, 15), (95, 0)), ((64, 0), (95, 15), (0, 15))      # (run e, pixel i): e = (c * 2 + dt) * 16 + dh; 63, 95: dt = 1
# the masked pixels of one token, as (run, pixel) pairs, and whether the token stays
V_SCENARIOS = (((V_PLUS[0],), True), ((V_PLUS[1],), True), ((V_PLUS[2],), True), ((V_ZERO[0],), False), ((V_ZERO[1],), False), ((V_ZERO[2],), False),
               ((V_PLUS[0], V_MINUS[0]), False), ((V_PLUS[1], V_MINUS[1]), False), ((V_PLUS[0], V_PLUS[1]), True), ((V_PLUS[2], V_PLUS[0]), True),
               ((V_MINUS[0], V_MINUS[1]), True))
V_TOKENS = ((0, 0, 0), (0, 0, 2), (0, 2, 0), (2, 0, 0), (3, 5, 5), (3, 5, 7), (3, 7, 5), (5, 5, 5), (7, 13, 13), (7, 13, 11), (2, 7, 0))   # (f, h, w): no two adjacent,


def video_w0_sign(seed=0):                            # so that every neighbour (in f, h, w) of a scenario token is an untouched patch that must stay kept
    g = G.gen(seed)
    w = torch.tensor([1, -1, 0], dtype=torch.int8)[torch.multinomial(torch.tensor([0.45, 0.45, 0.1]), 1536, True, generator=g)]
    for ks, v in ((V_PLUS, 1), (V_MINUS, -1), (V_ZERO, 0)):
        for e, i in ks:
            w[e * 16 + i] = v
    return w


def video_mask_cases(n_seg):
    """Content masks (n_seg, 16, 3, 224, 224) bool (True = kept) with V_SCENARIOS laid on V_TOKENS (segment n starts the scenario list n places later), and the
    expected token flags (n_seg, 1569) uint8 by construction (CLS kept; every token without a masked pixel kept)."""
    keep = torch.ones(n_seg, 16, 3, 224, 224, dtype=torch.bool)
    want = torch.ones(n_seg, 1569, dtype=torch.uint8)
    for n in range(n_seg):
        for j, (f, h, w) in enumerate(V_TOKENS):
            pix, stays = V_SCENARIOS[(j + n) % len(V_SCENARIOS)]
            for e, i in pix:
                c, dt, dh = e >> 5, (e >> 4) & 1, e & 15
                keep[n, f * 2 + dt, c, h * 16 + dh, w * 16 + i] = False
            want[n, 1 + f * 196 + h * 14 + w] = int(stays)
    return keep, want


def spec_w0_sign(seed=1):
    g = G.gen(seed)
    w = torch.tensor([1, -1, 0], dtype=torch.int8)[torch.multinomial(torch.tensor([0.45, 0.45, 0.1]), 256, True, generator=g)]
    w[torch.tensor([0, 17, 128])] = 1
    w[torch.tensor([255, 100])] = -1
    w[torch.tensor([15, 240, 136])] = 0
    return w


def spec_mask_cases(n_seg, F, Ta, seed):
    """Content masks (n_seg, F, Ta) bool: a few single masked pixels and pairs at random places (patches overlap, stride 10 under a 16-wide kernel: one pixel
    sits in up to four patches with a different weight in each).  The expectation comes from token_keep_literal."""
    g = G.gen(seed)
    keep = torch.ones(n_seg, F, Ta, dtype=torch.bool)
    n_pix = max(2, (F * Ta) // 160)
    for n in range(n_seg):
        keep[n, torch.randint(0, F, (n_pix,), generator=g), torch.randint(0, Ta, (n_pix,), generator=g)] = False
    return keep


def spec_token_keep(keep, w0, rule=token_keep_literal):
    """(n_seg, F, Ta) bool -> (n_seg, nf * nt + 2) uint8: tokens 0 and 1 (CLS, DISTILL) kept, the patches by `rule`."""
    n = keep.shape[0]
    body = rule(spec_patches(keep).view(n, -1, 256), w0.double())
    return torch.cat([torch.ones(n, 2, dtype=torch.uint8), body.to(torch.uint8)], 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# mel front-end
# ---------------------------------------------------------------------------------------------------------------------------------------------
MEL_FAMILIES = ('noise', 'gauss1e-4', 'gauss1e3', 'impulse0', 'impulse_last', 'silence', 'dc', 'tone100', 'tone440', 'tone7900')
MEL_TONAL = ('dc', 'tone100', 'tone440', 'tone7900')


def mel_wave(family, n_seg, n, seed):
    g = G.gen(seed)
    if family == 'noise':
        return torch.rand(n_seg, n, generator=g) * 2 - 1
    if family.startswith('gauss'):
        return torch.randn(n_seg, n, generator=g) * float(family[5:])
    w = torch.zeros(n_seg, n)
    if family == 'impulse0':
        w[:, 0] = 1.0 + torch.arange(n_seg)
    elif family == 'impulse_last':
        w[:, -1] = 1.0 + torch.arange(n_seg)
    elif family == 'dc':
        w += 0.5 + 0.25 * torch.arange(n_seg).unsqueeze(1)
    elif family.startswith('tone'):
        ph = torch.arange(n, dtype=torch.float64) * (2 * math.pi * float(family[4:]) / 16000.0)
        w = (0.5 * torch.sin(ph.unsqueeze(0) + torch.arange(n_seg, dtype=torch.float64).unsqueeze(1))).float()
    elif family != 'silence':
        raise ValueError(family)
    return w


def mel_frames(wave, n_frames, symmetric=False):
    """(n_seg, n) -> (n_seg, n_frames, 400): frame t = samples t * 160 - 200 + m of the reflect-padded segment (torch.stft center=True: the edge sample is not
    repeated).  symmetric: the defect 'reflection off by one' (the edge sample repeated)."""
    n = wave.shape[1]
    idx = torch.arange(n_frames).unsqueeze(1) * 160 - 200 + torch.arange(400).unsqueeze(0)
    lo, hi = (-idx - 1, 2 * n - 1 - idx) if symmetric else (-idx, 2 * (n - 1) - idx)
    idx = torch.where(idx < 0, lo, idx)
    idx = torch.where(idx >= n, hi, idx)
    return wave[:, idx]


def mel_consts(mean, std):
    """The kernel's fp32 constants: mean, inv = fl(1 / fl(2 std)), the floor fl(1e-6) and the padded frames' value fl(fl(0 - mean) * inv)."""
    m32 = np.float32(mean)
    inv = np.float32(1.0) / (np.float32(2.0) * np.float32(std))
    return dict(mean=float(m32), inv=float(inv), floor=float(np.float32(1e-6)), pad=float(np.float32(np.float32(0.0) - m32) * inv))


def mel_reference(wave, tables, pad_to, mean, std):
    """float64 log-mel of fp32 segments (n_seg, n) from the fp32 tables (dict of numpy arrays: tw_cos, tw_sin (400, 513), fb (513, n_mels), fb_lo, fb_hi) ->
    dict(ref, bar (n_seg, n_mels, pad_to) float64, frames = how many leading frames are computed (the rest: the pad value, bit for bit))."""
    k = mel_consts(mean, std)
    n = wave.shape[1]
    T = min(n // 160 + 1, pad_to)
    fr = mel_frames(wave.double(), T)
    tc, ts, fb = (torch.from_numpy(tables[x]).double() for x in ('tw_cos', 'tw_sin', 'fb'))
    n_k = torch.from_numpy(tables['fb_hi'] - tables['fb_lo']).double()
    re, im = fr @ tc, fr @ ts
    e_re, e_im = 401 * U32 * (fr.abs() @ tc.abs()), 401 * U32 * (fr.abs() @ ts.abs())
    P = re * re + im * im
    e_P = 2 * re.abs() * e_re + 2 * im.abs() * e_im + e_re * e_re + e_im * e_im + 3 * U32 * P
    A = P @ fb
    e_A = e_P @ fb + (n_k + 1) * U32 * A
    tot = A + k['floor']
    e_tot = e_A + U32 * tot
    v = torch.log(tot)
    down = torch.log(tot / torch.maximum(tot - e_tot, torch.full_like(tot, k['floor'] * (1 - U32))))
    e_v = torch.maximum(torch.log1p(e_tot / tot), down) + LOGF_ULP * 2.0 ** -23 * v.abs()
    out = (v - k['mean']) * k['inv']
    bar = e_v * k['inv'] + 3 * U32 * out.abs()
    n_seg, n_mels = wave.shape[0], fb.shape[1]
    ref = torch.full((n_seg, n_mels, pad_to), k['pad'], dtype=torch.float64)
    full = torch.zeros_like(ref)
    ref[:, :, :T], full[:, :, :T] = out.transpose(1, 2), bar.transpose(1, 2)
    return dict(ref=ref, bar=full, frames=T)


def _fma32(a, b, c):
    """fl32(a * b + c) on float64 carriers of fp32 values: the product of two fp32 numbers is exact in float64."""
    return (a * b + c).float().double()


def mel_emulate(wave, tables, pad_to, mean, std, symmetric=False, hi_short=False):
    """fp32 emulation of the two kernels in their own order: re / im by sequential fma over m = 0 .. 399, P = fl(fl(re re) + fl(im im)) - or with the product
    fused, which the compiler may choose: the criteria do not depend on it -, A by sequential fma over k in [fb_lo, fb_hi), fl(A + 1e-6f), log, fl(fl(v - mean) inv).
    symmetric / hi_short: the defects 'reflection off by one' and 'fb_hi one too small'.  -> (n_seg, n_mels, pad_to) fp32."""
    k = mel_consts(mean, std)
    n_seg, n = wave.shape
    T = min(n // 160 + 1, pad_to)
    fr = mel_frames(wave.float(), T, symmetric).double()
    tc, ts, fb = (torch.from_numpy(tables[x]).double() for x in ('tw_cos', 'tw_sin', 'fb'))
    lo, hi = torch.from_numpy(tables['fb_lo']).long(), torch.from_numpy(tables['fb_hi']).long() - int(hi_short)
    re = torch.zeros(n_seg, T, 513, dtype=torch.float64)
    im = torch.zeros_like(re)
    for m in range(400):
        x = fr[:, :, m:m + 1]
        re, im = _fma32(x, tc[m], re), _fma32(x, ts[m], im)
    P = _fma32(re, re, (im * im).float().double())
    A = torch.zeros(n_seg, T, fb.shape[1], dtype=torch.float64)
    for kk in range(int(lo.min()), int(hi.max())):
        live = (lo <= kk) & (kk < hi)
        A = torch.where(live, _fma32(P[:, :, kk:kk + 1], fb[kk], A), A)
    v = torch.log((A + k['floor']).float().double()).float().double()
    out = ((v - k['mean']).float().double() * k['inv']).float()
    res = torch.full((n_seg, fb.shape[1], pad_to), k['pad'], dtype=torch.float32)
    res[:, :, :T] = out.transpose(1, 2)
    return res


def mel_check(got, exp, emu=None):
    """The acceptance of one mel output (n_seg, n_mels, pad_to) fp32: the padded frames bit for bit, every computed element whose bar is at most MEL_CAP within
    its bar, and - with an emulation (the tonal families) - per (segment, frame) ||got - ref||_2 <= STAT_FACTOR ||emu - ref||_2 + ||bar_small||_2 over the mel
    axis, bar_small = the bar where it is at most MEL_CAP, 0 elsewhere.  Without an emulation every bar must be below MEL_CAP (so nothing is left out).
    -> dict(worst, share = the share of computed elements under the cap, frame = the worst per-frame ratio, msg)."""
    ref, bar, T = exp['ref'], exp['bar'], exp['frames']
    msgs = []
    pad_msg = bits_mismatch(got[:, :, T:].contiguous(), ref[:, :, T:].float().contiguous()) if T < ref.shape[2] else None
    if pad_msg:
        msgs.append('padded frames: ' + pad_msg)
    g, r, b = got[:, :, :T].double(), ref[:, :, :T], bar[:, :, :T]
    small = b <= MEL_CAP
    if emu is None and not small.all():
        msgs.append(f'bar up to {float(b.max()):.3g} exceeds the cap {MEL_CAP}: the family needs the per-frame criterion')
    el = elem_check(torch.where(small, g, r), r, b)
    if el['msg']:
        msgs.append(el['msg'])
    frame = 0.0
    if emu is not None:
        err = torch.nan_to_num((g - r), nan=INF).pow(2).sum(1).sqrt()
        lim = G.STAT_FACTOR * (emu[:, :, :T].double() - r).pow(2).sum(1).sqrt() + torch.where(small, b, torch.zeros_like(b)).pow(2).sum(1).sqrt()
        ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
        frame = float(ratio.max())
        for i in (~(ratio <= 1.0)).nonzero()[:3].tolist():
            msgs.append(f'segment {i[0]} frame {i[1]}: ||got - ref|| = {float(err[tuple(i)]):.4g} > limit {float(lim[tuple(i)]):.4g}')
    return dict(worst=el['worst'], share=float(small.double().mean()), frame=frame, msg='; '.join(msgs) if msgs else None)
