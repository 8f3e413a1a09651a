"""Host-side oracle of the weight-gradient GEMM tests (tests/test_wgrad_gemm_gpu.py), the train-step tail tests (tests/test_train_tail_gpu.py) and their CPU
screen (tests/test_train_tail_oracle_cpu.py): the case grids, float64 references computed from the very bf16 / fp32 values a kernel reads, fp32 emulations of a
correct kernel (each with the corruptions the CPU screen must see rejected), the derived error bars and one `*_verdict` per kernel that both the GPU tests and
the CPU screen call.  Nothing here touches a GPU API; every function works on the device its tensors live on.  Operand families, reference, emulation, the two
`wide` criteria, bf16_ulp and the canaries are gemm_oracle's.

Chain depths d (longest chain of dependent fp32 additions behind one output; where each was read is stated next to the function that returns it):
  sf_gemm_tn_splitk  part and bias_part  kc / 32 + 32      sf_gemm_tn_pp  part  kc / 16 + 16,  bias_part  kc / 2 + 1
  sf_softmax_rows  4 + 6      sf_softmax_bwd_rows  4 + 6      sf_colsum  colsum_depth()      sf_cross_entropy  ceil(C / 64) + 6 per row, B over rows
  sf_meanpool_l2norm768  t for the mean, 12 + 6 for the sum of squares      sf_similarity_f32  d      sf_reduce_groups_bf16  reduce_groups_depth()
A verdict returns a list of failure messages (empty = accepted) and, in `stats`, the worst error / bar it saw."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402

U32 = G.U32
MARGIN = G.MARGIN
TINY = 2.0 ** -126          # fp32 results below the smallest normal number may be flushed to zero by the hardware exponential / the denormal mode


def _f32(x):
    """A python float rounded to fp32 (what a `float` kernel argument holds), as a python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def _ratio(err, bar):
    return float(torch.nan_to_num(err / bar.clamp_min(1e-300), nan=float('inf')).max()) if err.numel() else 0.0


def within(got, ref, bar, what, stats=None, key=None):
    """[] when |got - ref| <= bar elementwise (a NaN fails), else one message; records the worst err / bar under stats[key]."""
    err = (got.double() - ref).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64, device=ref.device).expand_as(ref)
    bad = ~(err <= bar)
    r = _ratio(torch.where(bad & ~(err == err), torch.full_like(err, float('inf')), err), bar)
    if stats is not None:
        stats[key or what] = max(stats.get(key or what, 0.0), r)
    if not bad.any():
        return []
    i = bad.nonzero()[0].tolist()
    return [f'{what}: {int(bad.sum())} of {ref.numel()} elements outside the bar (worst err / bar {r:.3g}); first at {i}: got {got[tuple(i)].item()!r} '
            f'want {ref[tuple(i)].item()!r} bar {bar[tuple(i)].item()!r}']


def same_bits(got, want, what):
    bad = G.bits(got) != G.bits(want)
    if not bad.any():
        return []
    i = bad.nonzero()[0].tolist()
    return [f'{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise, first at {i}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}']


def damage(got, prefill, written, what):
    d = G.canary_damage(got, prefill, written)
    return [f'{what}: {d}'] if d else []


# =====================================================================================================================================================
# 1. weight-gradient GEMMs:  part[s] = dY[chunk s]^T X[chunk s]  (split, N, K) fp32,  bias_part[s] = sum_chunk dY  (split, N) fp32
#    gemm_oracle's A is dY_chunk^T (N x tokens), its W is X_chunk^T (K x tokens): the contraction runs over the token rows.
# =====================================================================================================================================================
TN_KSTEP = {'splitk': 32, 'pp': 16}            # tokens per MFMA: v_mfma_f32_16x16x32_bf16 (sf_gemm.hip, gemm_tn_splitk_kernel) / v_mfma_f32_32x32x16_bf16 (sf_gemm_tn_pp.hip)
TN_MFMA = {'splitk': '16x16x32', 'pp': '32x32x16'}
TN_TILE = {'splitk': 128, 'pp': 256}
TN_PAD_ROWS = 5                                 # NaN token rows behind row M - 1 of both operands
TN_LD_EXTRA = (64, 8)                           # dY is the column slice [64:] of a buffer 64 wider, X the slice [:K] of one 8 wider

# (family, M, N, K, split, kc): k-tiles of 32 per chunk nk in {0, 1, 2, 3, 4, 5, 6, 9, 10}, valid % 32 of the last non-empty chunk in {1, 3, 5, 31}, tile counts 1, 3, 3, 9, 12
TN_SPLITK_CASES = [
    ('exact', 65, 128, 128, 4, 64),             # chunks of 64 | 1 | 0 | 0 rows: nk 2, 1, 0, 0 (a prologue shorter than the ring; two empty chunks)
    ('wide', 101, 128, 128, 3, 64),             # 64 | 37 | 0: nk 2, 2 (valid % 32 = 5), 0
    ('exact', 195, 128, 384, 3, 128),           # 128 | 67 | 0: nk 4 (prologue 3 + one refill), 3 (exactly the prologue; valid % 32 = 3), 0
    ('wide', 325, 384, 128, 2, 192),            # 192 | 133: nk 6, 5 (valid % 32 = 5): the ring wraps
    ('wide', 607, 384, 384, 3, 320),            # 320 | 287 | 0: nk 10, 9 (valid % 32 = 31), 0: tm > 0 and tn > 0 under the XCD remap of 9 tiles
    ('exact', 287, 256, 768, 4, 128),           # 128 | 128 | 31 | 0: nk 4, 4, 1 (valid = 31), 0; 12 tiles
    ('wide', 227, 256, 768, 4, 64),             # 64 | 64 | 64 | 35: nk 2, 2, 2, 2 (valid % 32 = 3)
    ('exact', 225, 384, 384, 2, 128),           # 128 | 97: nk 4, 4 (valid % 32 = 1)
    ('exact', 192, 384, 384, 3, 64),            # 64 | 64 | 64: every chunk full (no ragged tile at all)
    ('marker', 261, 128, 384, 3, 192),          # 192 | 69 | 0
]
# last chunk of 1, 63, 65 and kc - 1 rows (whole 64-row k-tiles past M included); items = tiles * split in {1, 4, 4, 6, 6, 7, 9, 11, 12}
TN_PP_CASES = [
    ('exact', 1, 256, 256, 1, 128),             # 1 item: seven XCDs empty, every workgroup but one returns before any barrier; k-tile 1 entirely past M
    ('wide', 6 * 256 + 63, 256, 256, 7, 256),   # 7 items: one empty XCD
    ('exact', 8 * 384 + 65, 256, 256, 9, 384),  # 9 items: per = 2, the last XCD range holds one item, three XCDs are empty
    ('wide', 10 * 128 + 127, 256, 256, 11, 128),   # 8 + 3 items, last chunk kc - 1 rows
    ('exact', 256 + 255, 512, 256, 2, 256),     # tm > 0
    ('wide', 384 + 1, 256, 512, 2, 384),        # tn > 0; 5 of the last chunk's 6 k-tiles entirely past M
    ('exact', 128 + 63, 512, 768, 2, 128),      # 12 items, tm > 0 and tn > 0
    ('wide', 65, 512, 768, 1, 256),             # one chunk of 65 rows: k-tiles 2 and 3 empty
    ('marker', 2 * 256 + 191, 256, 512, 3, 256),
]


def tn_pp_walk_cases(blocks):
    """The two item walks of sf_gemm_tn_pp at N = K = 256, kc = 128 (one tile per chunk: items = split) for a launch of `blocks` workgroups (n_cu & ~7): items
    just above `blocks` - some workgroups take two items - and above 2 * blocks - some take three."""
    return [('exact', (blocks + 4) * 128 + 77, 256, 256, blocks + 5, 128), ('exact', (2 * blocks + 8) * 128 + 65, 256, 256, 2 * blocks + 9, 128)]


def tn_depth(kernel, kc):
    """part: one MFMA per k-step of the chunk behind each accumulator (gemm_tn_splitk_kernel's kt loop, sf_gemm.hip; gemm_tn_pp_kernel's mma(), 4 k-steps per
    phase, sf_gemm_tn_pp.hip) + the depth of one MFMA."""
    return G.depth(kc, TN_MFMA[kernel])


def tn_bias_depth(kernel, kc):
    """bias_part.  tn_splitk: one more MFMA (against all-ones) per k-step into accb[] - the same chain as part.  tn_pp: bias_acc() adds, per 64-token k-tile, 4
    fragments x 4 v_dot2_f32_bf16 (two additions each) into one bsum[] per lane = kc / 2 additions, then one cross-half add (__shfl_xor 32) in the epilogue."""
    return G.depth(kc, TN_MFMA[kernel]) if kernel == 'splitk' else kc // 2 + 1


def tn_operands(family, M, N, K, seed):
    """dY (M + TN_PAD_ROWS, N) and X (M + TN_PAD_ROWS, K) bf16, token-major; rows beyond M hold NaN.  exact / wide are gemm_oracle's families generated as
    (N x tokens) and (K x tokens) and transposed, so `wide` changes magnitude per 32-token block and per column.  marker: dY[m, i] = 1 iff i == m mod N and X
    carries a code of the token row (even columns m % 251 + 1, odd columns m // 251 + 1), so part[s][i] is the sum of the codes of chunk s's rows m = i mod N."""
    rows = M + TN_PAD_ROWS
    if family == 'marker':
        m = torch.arange(M)
        dy = torch.zeros(M, N)
        dy[m, m % N] = 1.0
        x = torch.where(torch.arange(K)[None, :] % 2 == 0, (m % 251 + 1)[:, None], (m // 251 + 1)[:, None]).float().expand(M, K)
    else:
        T = -(-M // 32) * 32
        o = G.operands(family, N, K, T, seed, a_rows=N)
        dy, x = o['a'].float().t()[:M], o['w'].float().t()[:M]
    dyb, xb = torch.full((rows, N), float('nan')), torch.full((rows, K), float('nan'))
    dyb[:M], xb[:M] = dy, x
    return dyb.bfloat16(), xb.bfloat16()


def tn_exact_bound(dy, x, M, kc):
    """An upper bound of every partial sum of |dy x| inside one chunk (and of the bias sums): exactness of the integer families needs it below 2^24."""
    return kc * float(dy[:M].float().abs().max()) * max(float(x[:M].float().abs().max()), 1.0)


def tn_chunks(M, split, kc):
    return [(min(M, s * kc), min(M, (s + 1) * kc)) for s in range(split)]


def tn_reference(dy, x, M, split, kc):
    """float64 part (split, N, K), S = sum |dy x|, bias (split, N), Sb = sum |dy| per chunk, from the bf16 values; an empty chunk is zero."""
    N, K = dy.shape[1], x.shape[1]
    part, S = torch.zeros(split, N, K, dtype=torch.float64, device=dy.device), torch.zeros(split, N, K, dtype=torch.float64, device=dy.device)
    bias, Sb = torch.zeros(split, N, dtype=torch.float64, device=dy.device), torch.zeros(split, N, dtype=torch.float64, device=dy.device)
    for s, (lo, hi) in enumerate(tn_chunks(M, split, kc)):
        if hi > lo:
            part[s], S[s] = G.reference(dy[lo:hi].t(), x[lo:hi].t())
            bias[s], Sb[s] = dy[lo:hi].double().sum(0), dy[lo:hi].double().abs().sum(0)
    return part + 0.0, S, bias + 0.0, Sb        # a kernel accumulates onto +0: a sum of nothing but -0 products is +0 there, and x + 0.0 makes it so here


TN_MUTATIONS = ('drop_last_row', 'read_row_M', 'neighbour_chunk', 'ktile_twice', 'swap_chunks', 'bias_tile1', 'empty_unwritten')


def tn_emulate(kernel, dy, x, M, split, kc, mutate=None):
    """fp32 emulation of a correct kernel: per chunk, the k-steps of TN_KSTEP tokens accumulated one after another (gemm_oracle.emulate); the bias sums the same way
    (tn_splitk: against ones) or, for tn_pp, as two per-lane chains of pair sums over the token halves of every 16-token step + one add.  `mutate`: one of
    TN_MUTATIONS.  Returns part (split, N, K), bias (split, N) fp32; an unwritten chunk keeps gemm_oracle's canary."""
    ks, tile = TN_KSTEP[kernel], TN_TILE[kernel]
    N, K = dy.shape[1], x.shape[1]
    dyf, xf = torch.nan_to_num(dy.float()[:M + 1], nan=1.0), torch.nan_to_num(x.float()[:M + 1], nan=1.0)     # row M: what a kernel reading it would see, non-zero
    chunks = tn_chunks(M, split, kc)
    last = max(s for s, (lo, hi) in enumerate(chunks) if hi > lo)
    part, bias = G.canary((split, N, K), torch.float32), G.canary((split, N), torch.float32)
    for s, (lo, hi) in enumerate(chunks):
        if hi == lo and mutate == 'empty_unwritten':
            continue
        rows = torch.arange(lo, hi)
        if s == last and mutate == 'drop_last_row':
            rows = rows[:-1]
        if s == last and mutate == 'read_row_M':
            assert hi - lo < kc, 'the mutation needs a ragged chunk'
            rows = torch.cat([rows, torch.tensor([M])])
        if mutate == 'neighbour_chunk' and s in (0, 1):
            assert chunks[1][1] > chunks[1][0], 'the mutation needs two non-empty chunks'
            rows = torch.cat([rows, torch.tensor([chunks[1][0]])]) if s == 0 else rows[1:]
        a, w = dyf[rows], xf[rows].clone()
        if mutate == 'swap_chunks' and s == 0:
            w[1, 0:8], w[1, 8:16] = xf[rows[1], 8:16], xf[rows[1], 0:8]
        pad = -len(rows) % ks
        a, w = torch.nn.functional.pad(a, (0, 0, 0, pad)), torch.nn.functional.pad(w, (0, 0, 0, pad))
        nblk = a.shape[0] // ks
        order = list(range(nblk))
        if mutate == 'ktile_twice' and s == 0:
            order = [0] + order
        part[s] = G.emulate(a.t(), w.t(), None, None, gelu=False, out_bf16=False, kblock=ks, kblocks=order) if nblk else 0.0
        ab = a.roll(-tile, 1) if mutate == 'bias_tile1' else a
        if kernel == 'splitk' or not nblk:
            bias[s] = G.emulate(ab.t(), torch.ones(1, a.shape[0]), None, None, gelu=False, out_bf16=False, kblock=ks, kblocks=order)[:, 0] if nblk else 0.0
        else:
            pairs = ab.view(nblk, 2, 4, 2, N)                          # [16-token step][token half = lane group][pair][2]
            h = torch.zeros(2, N)
            for k in order:
                for q in range(4):
                    h = h + (pairs[k, :, q, 0] + pairs[k, :, q, 1])
            bias[s] = h[0] + h[1]
    return part, bias


def tn_marker_report(dy, x, M, split, kc, got_part):
    """For the marker case: which token rows are behind the first wrong rows of part."""
    N = dy.shape[1]
    ref = tn_reference(dy, x, M, split, kc)[0]
    bad = (got_part.double() != ref).any(2)
    out = []
    for s, i in bad.nonzero()[:4].tolist():
        lo, hi = tn_chunks(M, split, kc)[s]
        toks = [m for m in range(lo, hi) if m % N == i]
        out.append(f'chunk {s} output row {i} (token rows {toks}): codes got {got_part[s, i, :2].tolist()} want {ref[s, i, :2].tolist()}')
    return out


def tn_verdict(kernel, family, dy, x, M, split, kc, got_part, got_bias, stats=None):
    """Failure messages of one launch's part (split, N, K) and bias_part (split, N) - None for a launch without it - (fp32, same device as dy / x)."""
    stats = {} if stats is None else stats
    ref, S, bref, Sb = tn_reference(dy, x, M, split, kc)
    msgs = []
    if family in ('exact', 'marker'):
        assert tn_exact_bound(dy, x, M, kc) < 2 ** 24
        m = G.exact_mismatch(got_part.reshape(-1, got_part.shape[-1]), ref.reshape(-1, ref.shape[-1]), False)
        if m:
            msgs.append(f'part (rows are s * N + i): {m}')
            if family == 'marker':
                msgs += tn_marker_report(dy, x, M, split, kc, got_part)
        if got_bias is not None:
            m = G.exact_mismatch(got_bias, bref, False)
            if m:
                msgs.append(f'bias_part: {m}')
        return msgs
    emu_p, emu_b = tn_emulate(kernel, dy.cpu(), x.cpu(), M, split, kc)
    exp = G.expected(ref, S, None, gelu=False, out_bf16=False, d=tn_depth(kernel, kc))
    for s in range(split):
        c = G.wide_check(got_part[s], {k: v[s] for k, v in exp.items()}, emu_p[s].to(dy.device))
        stats['part elem'], stats['part stat'] = max(stats.get('part elem', 0.0), c['elem']), max(stats.get('part stat', 0.0), c['stat'])
        if c['msg']:
            msgs.append(f'part[{s}]: {c["msg"]}')
    if got_bias is not None:
        c = G.wide_check(got_bias, G.expected(bref, Sb, None, gelu=False, out_bf16=False, d=tn_bias_depth(kernel, kc)), emu_b.to(dy.device))
        stats['bias elem'], stats['bias stat'] = max(stats.get('bias elem', 0.0), c['elem']), max(stats.get('bias stat', 0.0), c['stat'])
        if c['msg']:
            msgs.append(f'bias_part: {c["msg"]}')
    return msgs


# =====================================================================================================================================================
# 2. sf_softmax_rows / sf_softmax_bwd_rows
# =====================================================================================================================================================
SOFTMAX_L = [1, 63, 64, 65, 198, 255, 256]
SOFTMAX_ROWS = [1, 5, 8]
SOFTMAX_SCALES = [0.125, 1.0]
SOFTMAX_KINDS = ['flat', 'sharp', 'spread', 'shifted']
SOFTMAX_DEPTH = 4 + 6           # softmax_rows_kernel / softmax_bwd_rows_kernel (sf_train.hip): 4 terms per lane in sequence, then wave_sum's 6 butterfly levels


def softmax_lpads(L):
    return sorted({L, -(-L // 32) * 32, 256})


def softmax_logits(kind, rows, L, scale, seed):
    """fp32 logits S (rows, L): flat - all equal; sharp - one logit 30 / scale above the rest; spread - scale * (S - max) from 0 down to -80; shifted - the spread
    row plus 10^4 / scale."""
    g = G.gen(seed)
    if kind == 'flat':
        return torch.full((rows, L), 1.75)
    if kind == 'sharp':
        s = torch.randn(rows, L, generator=g) * 0.01
        s[torch.arange(rows), torch.randint(0, L, (rows,), generator=g)] += 30.0 / scale
        return s
    s = -80.0 * torch.rand(rows, L, generator=g) / scale
    s[torch.arange(rows), torch.randint(0, L, (rows,), generator=g)] = 0.0
    if L > 1:
        s[:, (L // 2 + 1) % L] = torch.where(s[:, (L // 2 + 1) % L] == 0.0, s[:, (L // 2 + 1) % L], torch.full((rows,), -80.0 / scale))
    return s + 1e4 / scale if kind == 'shifted' else s


def softmax_reference(S, scale):
    """float64 p = softmax(scale * S) and F, the fp32 term of the forward bar, from the fp32 logits and the fp32 scale the kernel receives:
    per element the relative error  e_j = 2^-23 (v_exp_f32: 1 ulp, the ISA's documented accuracy - not derivable from the kernel's code) + |x_j - m| 2^-23 (the
    rounding of the exponential's argument: the subtraction and __expf's product with log2 e) + the rounding of x = scale * S and of m where that product is not exact
    (nothing for a power-of-two scale);  the sum carries sum_j p_j e_j + (4 + 6) 2^-24, the reciprocal and the product one rounding each:
    F = p (e_i + sum_j p_j e_j + (10 + 2) 2^-24) + 2^-126 (a result below the normal range may be flushed)."""
    x = S.double() * _f32(scale)
    m = x.amax(1, keepdim=True)
    e = torch.exp(x - m)
    p = e / e.sum(1, keepdim=True)
    rx = (x - x.float().double()).abs()
    ej = 2 * U32 + (x - m).abs() * 2 * U32 + rx + rx.amax(1, keepdim=True)
    F = p * (ej + (p * ej).sum(1, keepdim=True) + (SOFTMAX_DEPTH + 2) * U32) + TINY
    return p, F


def softmax_emulate(S, scale, L_pad, mutate=None):
    """fp32 emulation -> bf16 P (rows, L_pad).  mutate: 'no_max' (no max subtraction), 'norm_lpad' (the pad columns counted in the sum, as copies of the row's last logit), 'rtz'."""
    v = S.float() * _f32(scale)
    L = S.shape[1]
    m = torch.zeros(S.shape[0], 1) if mutate == 'no_max' else v.amax(1, keepdim=True)
    e = torch.exp(v - m)
    s = e.sum(1, keepdim=True)
    if mutate == 'norm_lpad':
        s = s + (L_pad - L) * e[:, -1:]
    p = G.round_bf16(e * (1.0 / s), rtz=mutate == 'rtz')
    return torch.nn.functional.pad(p, (0, L_pad - L)).bfloat16()


def softmax_verdict(S, scale, L_pad, got, prefill, stats=None):
    """got / prefill: the whole (rows, ld) bf16 buffer after / before the launch."""
    L = S.shape[1]
    p, F = softmax_reference(S, scale)
    msgs = within(got[:, :L].float(), p, G.bf16_ulp(p) / 2 + F, 'softmax P', stats, 'softmax fwd')
    if L_pad > L:
        msgs += same_bits(got[:, L:L_pad], torch.zeros_like(got[:, L:L_pad]), 'softmax pad columns')
    written = torch.zeros_like(got, dtype=torch.bool)
    written[:, :L_pad] = True
    return msgs + damage(got, prefill, written, 'softmax P')


def softmax_bwd_reference(P, dP, scale):
    """float64 dS = scale P (dP - sum_j P_j dP_j) from the bf16 P and fp32 dP the kernel reads, and the fp32 term's scale  scale p (|dP| + sum |p dP|)."""
    p, g, sc = P.double(), dP.double(), _f32(scale)
    dot = (p * g).sum(1, keepdim=True)
    return sc * p * (g - dot), sc * p * (g.abs() + (p * g).abs().sum(1, keepdim=True))


def softmax_bwd_dp(P, seed):
    """fp32 dP (rows, L) for the bf16 P (rows, L) the backward reads; the kind goes by the row index: r % 3 == 0 Gaussian; 1 constant 3, so that dP - sum p dP cancels to
    the rounding of P; 2 the dot product itself cancels - dP_j = +1 / p_j, -1 / p_j in pairs (0 for the unpaired last element of an odd L), every |p_j dP_j| = 1 and
    |sum p dP| <= 1e-6 sum |p dP|: the row in which the bar's sum |p dP| term, not |sum p dP|, carries the error."""
    rows, L = P.shape
    dP = torch.randn(rows, L, generator=G.gen(seed))
    sign = torch.where(torch.arange(L) % 2 == 0, 1.0, -1.0)
    if L % 2:
        sign[-1] = 0.0
    for r in range(rows):
        if r % 3 == 1:
            dP[r] = 3.0
        elif r % 3 == 2:
            dP[r] = sign / P[r].float().clamp_min(1e-37)
    return dP


def softmax_bwd_emulate(P, dP, scale, L_pad, mutate=None):
    p, g = P.float(), dP.float()
    dot = (p * g).sum(1, keepdim=True)
    if mutate == 'drop_last_term':
        dot = dot - p[:, -1:] * g[:, -1:]
    return torch.nn.functional.pad(_f32(scale) * p * (g - dot), (0, L_pad - P.shape[1])).bfloat16()


def softmax_bwd_verdict(P, dP, scale, L_pad, got, prefill, stats=None):
    L = P.shape[1]
    ref, T = softmax_bwd_reference(P, dP, scale)
    msgs = within(got[:, :L].float(), ref, G.bf16_ulp(ref) / 2 + MARGIN * (SOFTMAX_DEPTH + 3) * U32 * T + TINY, 'softmax dS', stats, 'softmax bwd')
    if L_pad > L:
        msgs += same_bits(got[:, L:L_pad], torch.zeros_like(got[:, L:L_pad]), 'softmax dS pad columns')
    written = torch.zeros_like(got, dtype=torch.bool)
    written[:, :L_pad] = True
    return msgs + damage(got, prefill, written, 'softmax dS')


# =====================================================================================================================================================
# 3. sf_colsum
# =====================================================================================================================================================
COLSUM_ROWS = [1, 63, 64, 65, 1000, 16383, 16384, 16385]
COLSUM_COLS = [21, 32, 64, 96, 768]


def colsum_rpb(rows):
    return 256 if rows >= 16384 else 64        # sf_colsum (sf_train.hip): rows per first-stage block


def colsum_is_vec(cols, bf16, aligned):
    """sf_colsum takes the vector kernel when cols is a multiple of 32 (fp32) / 64 (bf16) and base pointer and row stride are 16-byte aligned."""
    return aligned and cols % (64 if bf16 else 32) == 0


def colsum_depth(rows, vec):
    """First stage: colsum_stage1_kernel adds the block's rpb rows in sequence; colsum_stage1_vec_kernel rpb / 32 rows per lane, then 3 shuffle levels and 2 levels
    over the four waves.  Second stage (colsum_partials_kernel): ceil(nblk / 64) + 3 per accumulator, 2 levels, 16 lane groups in sequence, + the accumulate add."""
    rpb = colsum_rpb(rows)
    nblk = -(-rows // rpb)
    return (rpb // 32 + 3 + 2 if vec else rpb) + -(-nblk // 64) + 3 + 2 + 16 + 1


def colsum_workspace(rows, cols):
    return cols * -(-rows // 64)               # the header's contract


def colsum_emulate(x, mutate=None):
    rows, rpb = x.shape[0], colsum_rpb(x.shape[0])
    blocks = [x[r:r + rpb].float().sum(0) for r in range(0, rows, rpb)]
    if mutate == 'drop_last_block' and len(blocks) > 1:
        blocks = blocks[:-1]
    return torch.stack(blocks).sum(0)


def colsum_verdict(x, prefill, accumulate, vec, got, stats=None):
    """x (rows, cols) fp32 | bf16 as the kernel reads it; prefill / got (cols,) fp32.  c = 1: the rounding of the last addition."""
    xd = x.double()
    ref, T = xd.sum(0), xd.abs().sum(0)
    if accumulate:
        ref, T = ref + prefill.double(), T + prefill.double().abs()
    return within(got, ref, (colsum_depth(x.shape[0], vec) + 1) * U32 * T, 'colsum', stats, 'colsum')


# =====================================================================================================================================================
# 4. sf_cross_entropy
# =====================================================================================================================================================
CE_B = [1, 16, 33]
CE_C = [1, 2, 21, 64, 65, 130]
CE_KINDS = ['gauss', 'spread', 'offset']


def ce_logits(kind, B, C, seed):
    g = G.gen(seed)
    z = torch.randn(B, C, generator=g)
    if kind == 'spread':
        z = (torch.rand(B, C, generator=g) * 2 - 1) * 80.0
    if kind == 'offset':
        z = z + 1e4
    return z, torch.randint(0, C, (B,), generator=g)


def ce_reference(z, tgt, grad_scale):
    """float64 loss, gradient and their bars.  Per row (cross_entropy_kernel, sf_train.hip): s = sum exp(z - m) carries e_s = sum_j p_j e_j + (ceil(C / 64) + 6) 2^-24
    with e_j = 2^-23 (1 + |z_j - m|) as in softmax_reference; logf one ulp, (m + log s) - z_t two roundings, the running total B additions of at most B mean|loss_b|,
    one division:  loss bar = (5 + B) 2^-24 mean_b(|m| + |log s| + |z_t|) + mean_b e_s.
    gradient: p_j carries e_j + e_s + one division, (p - onehot) one subtraction, grad_scale / B and the product one rounding each:
    bar = (grad_scale / B) 2^-24 (p (e_j + e_s) / 2^-24 + p + 3 |p - onehot|) + 2^-126."""
    B, C = z.shape
    zd = z.double()
    m = zd.amax(1, keepdim=True)
    e = torch.exp(zd - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    zt = zd[torch.arange(B), tgt]
    loss = (m[:, 0] + torch.log(s[:, 0]) - zt).mean()
    ej = 2 * U32 * (1 + (zd - m).abs())
    es = (p * ej).sum(1, keepdim=True) + (-(-C // 64) + 6) * U32
    loss_bar = (5 + B) * U32 * (m[:, 0].abs() + torch.log(s[:, 0]).abs() + zt.abs()).mean() + es.mean()
    onehot = torch.zeros_like(zd)
    onehot[torch.arange(B), tgt] = 1.0
    gs = _f32(grad_scale)
    grad = (p - onehot) * (gs / B)
    grad_bar = (gs / B) * (p * (ej + es) + U32 * (p + 3 * (p - onehot).abs())) + TINY
    return loss, loss_bar, grad, grad_bar


def ce_emulate(z, tgt, grad_scale, mutate=None):
    B = z.shape[0]
    zf = z.float()
    m = zf.amax(1, keepdim=True)
    e = torch.exp(zf - m)
    s = e.sum(1, keepdim=True)
    loss = ((m[:, 0] + torch.log(s[:, 0])) - zf[torch.arange(B), tgt]).sum() / B
    onehot = torch.zeros_like(zf)
    onehot[torch.arange(B), tgt] = 1.0
    return loss, (e / s - onehot) * (_f32(grad_scale) / (1 if mutate == 'no_div_B' else B))


def ce_verdict(z, tgt, grad_scale, got_loss, got_grad, stats=None):
    """got_grad: (B, C) or None (dlogits = NULL)."""
    loss, loss_bar, grad, grad_bar = ce_reference(z, tgt, grad_scale)
    msgs = within(got_loss.reshape(()), loss, loss_bar, 'cross-entropy loss', stats, 'ce loss')
    if z.shape[1] == 1:
        msgs += same_bits(got_loss.reshape(1), torch.zeros(1), 'cross-entropy loss at C = 1')
    if got_grad is not None:
        msgs += within(got_grad, grad, grad_bar, 'cross-entropy gradient', stats, 'ce grad')
        if z.shape[1] == 1:
            msgs += same_bits(got_grad, torch.zeros_like(got_grad), 'cross-entropy gradient at C = 1')
    return msgs


# =====================================================================================================================================================
# 5. sf_adam_clip_step
# =====================================================================================================================================================
ADAM_N = [1, 255, 256, 257, 100003]
ADAM_STEPS = [1, 2, 1000, 100000]
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_K_M, ADAM_K_V = 6, 10


def adam_reference(p, g, m, v, norm, max_norm, step, hp=ADAM_HP):
    """float64 Adam step from the fp32 p, g, m, v, the norm in the buffer and the FP32-ROUNDED lr, beta1, beta2, eps, max_norm the kernel receives (bias
    corrections 1 - beta^step of those values).  Returns dict(m, v, m_bar, v_bar, coef, b1, b2, lr, eps, bc1, bc2, bc_rel).
    m = beta1 m + (1 - beta1) (g coef): coef = min(1, max_norm / (norm + 1e-6)) two roundings, g coef one, (1 - beta1) is exact (Sterbenz), two products and one
    addition -> ADAM_K_M = 6 roundings on the sum of the two terms' magnitudes; v: the square doubles the three of g coef, + 1 + 3 -> ADAM_K_V = 10."""
    lr, b1, b2, eps = (_f32(hp[k]) for k in ('lr', 'beta1', 'beta2', 'eps'))
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, _f32(max_norm) / (float(norm) + _f32(1e-6)))
    gd = g.double() * coef
    t1, t2 = b1 * m.double(), (1 - b1) * gd
    u1, u2 = b2 * v.double(), (1 - b2) * gd * gd
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    # the launcher computes 1.0f - powf(beta, step) in fp32: powf within 2 ulp of beta^step, the subtraction one rounding -> relative error of bc
    bc_rel = [(2 * 2 * U32 * b ** step + U32 * bc) / bc for b, bc in ((b1, bc1), (b2, bc2))]
    return dict(m=t1 + t2, v=u1 + u2, m_bar=ADAM_K_M * U32 * (t1.abs() + t2.abs()), v_bar=ADAM_K_V * U32 * (u1.abs() + u2.abs()), coef=coef, lr=lr, eps=eps,
                bc1=bc1, bc2=bc2, bc_rel=bc_rel)


def adam_p_reference(p, m_new, v_new, r):
    """p' = p - dp, dp = lr (m / bc1) / (sqrt(v / bc2) + eps) in float64 from the m and v the kernel RETURNED (held to their own bars separately, so that their
    cancellation does not enter p's bar).  Roundings behind dp (adam_clip_kernel, sf_train.hip): m / bc1, v / bc2 (half through the root), sqrt, + eps, lr *, the
    last division = k = 6, plus bc1's and half of bc2's relative error from the launcher; the final subtraction rounds p':  bar = 2^-24 |p'| + (k 2^-24 + e_bc) |dp|."""
    dp = r['lr'] * (m_new.double() / r['bc1']) / (torch.sqrt(v_new.double() / r['bc2']) + r['eps'])
    ref = p.double() - dp
    return ref, U32 * ref.abs() + (6 * U32 + r['bc_rel'][0] + 0.5 * r['bc_rel'][1]) * dp.abs() + TINY


def adam_emulate(p, g, m, v, norm, max_norm, step, hp=ADAM_HP, mutate=None):
    """fp32 emulation -> p', m', v'.  mutate: 'swap_bc' (bias corrections swapped), 'clip_after' (the clip coefficient applied after the moment update)."""
    f = lambda t: torch.tensor(t, dtype=torch.float32)
    lr, b1, b2, eps = (f(hp[k]) for k in ('lr', 'beta1', 'beta2', 'eps'))
    coef = torch.minimum(f(1.0), f(max_norm) / (norm.float() + f(1e-6))) if max_norm > 0 else f(1.0)
    gi = g if mutate == 'clip_after' else g * coef
    mi = b1 * m + (1 - b1) * gi
    vi = b2 * v + (1 - b2) * gi * gi
    bc1, bc2 = 1 - torch.pow(b1, f(float(step))), 1 - torch.pow(b2, f(float(step)))
    if mutate == 'swap_bc':
        bc1, bc2 = bc2, bc1
    upd = lr * (mi / bc1) / (torch.sqrt(vi / bc2) + eps)
    return p - (upd * coef if mutate == 'clip_after' else upd), mi, vi


def adam_verdict(p, g, m, v, norm, max_norm, step, got_p, got_m, got_v, got_pb, stats=None):
    """p, g, m, v: the (n,) fp32 inputs; got_*: the outputs (got_pb the bf16 copy or None)."""
    r = adam_reference(p, g, m, v, norm, max_norm, step)
    msgs = within(got_m, r['m'], r['m_bar'] + TINY, 'adam m', stats, 'adam m') + within(got_v, r['v'], r['v_bar'] + TINY, 'adam v', stats, 'adam v')
    ref, bar = adam_p_reference(p, got_m, got_v, r)
    msgs += within(got_p, ref, bar, 'adam p', stats, 'adam p')
    if got_pb is not None:
        msgs += same_bits(got_pb, got_p.bfloat16(), 'adam p_bf16 vs RNE of the returned p')
    return msgs


# =====================================================================================================================================================
# 6. Stage-1 head and tower-backward helper
# =====================================================================================================================================================
POOL_N, POOL_T = [1, 3, 4, 5], [1, 6, 8]
POOL_SS_DEPTH = 12 + 6          # meanpool_l2norm768_kernel (sf_clip.hip) / its _bwd (sf_towerbwd.hip): 12 squares per lane in sequence + wave_sum's 6 levels


def meanpool_reference(x, t, normalize):
    """x (n * t, 768) fp32 -> float64 y (n, 768) and its bar.  mean: t additions in sequence, 1 / t and the product -> em = (t + 2) 2^-24 sum_j |x_j| / t per element.
    normalize: y = m / nrm, nrm = max(||m||, 1e-12): the sum of squares is 12 + 6 deep with one rounding per square -> nrm carries sum |m| em / nrm^2 + ((18 + 1) / 2 + 1)
    2^-24 relative (the root halves the sum's, + its own rounding), the reciprocal and the product one rounding each:
    bar = MARGIN (em / nrm + |y| (sum_k |m_k| em_k / nrm^2 + 13 2^-24)).  Pooled-row norms stay inside [1e-15, 1e15]: the fp32 sum of squares leaves the normal range outside
    it (and its terms, ||m||^2 / 768, before that), exactly as in the reference's fp32 F.normalize - nothing to hold a kernel to there."""
    n = x.shape[0] // t
    xd = x.double().view(n, t, -1)
    m = xd.sum(1) / t
    em = (t + 2) * U32 * xd.abs().sum(1) / t
    if not normalize:
        return m, MARGIN * em + TINY
    nrm = m.norm(dim=1, keepdim=True).clamp_min(1e-12)
    y = m / nrm
    e_n = (m.abs() * em).sum(1, keepdim=True) / (nrm * nrm) + ((POOL_SS_DEPTH + 1) / 2 + 1) * U32
    return y, MARGIN * (em / nrm + y.abs() * (e_n + 2 * U32)) + TINY


def meanpool_emulate(x, t, normalize, mutate=None):
    n = x.shape[0] // t
    m = x.float().view(n, t, -1).sum(1) * (1.0 / (t + 1 if mutate == 't_plus_1' else t))
    return m / m.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else m


def meanpool_bwd_reference(x, dy, t, normalize):
    """float64 dx (n * t, 768) and its bar: dx = (dy / nrm - m <m, dy> / nrm^3) / t.  With e_n (units of 1) the relative error of nrm as in meanpool_reference and
    e_dot = (18 + 1) 2^-24 sum |m dy| + sum em |dy| the absolute error of the dot product:
    bar = MARGIN / t (|dy| / nrm (e_n + 4 2^-24) + (em |dot| + |m| e_dot) / nrm^3 + |m| |dot| / nrm^3 (3 e_n + 6 2^-24));  normalize = 0: dx = dy / t, two roundings."""
    n = x.shape[0] // t
    g = dy.double()
    if not normalize:
        dm, bar = g / t, 2 * U32 * g.abs() / t
    else:
        xd = x.double().view(n, t, -1)
        m = xd.sum(1) / t
        em = (t + 2) * U32 * xd.abs().sum(1) / t
        nrm = m.norm(dim=1, keepdim=True).clamp_min(1e-12)
        e_n = (m.abs() * em).sum(1, keepdim=True) / (nrm * nrm) + ((POOL_SS_DEPTH + 1) / 2 + 1) * U32
        dot = (m * g).sum(1, keepdim=True)
        e_dot = (POOL_SS_DEPTH + 1) * U32 * (m * g).abs().sum(1, keepdim=True) + (em * g.abs()).sum(1, keepdim=True)
        dm = (g / nrm - m * dot / nrm ** 3) / t
        bar = (g.abs() / nrm * (e_n + 4 * U32) + (em * dot.abs() + m.abs() * e_dot) / nrm ** 3 + m.abs() * dot.abs() / nrm ** 3 * (3 * e_n + 6 * U32)) / t
    return dm.repeat_interleave(t, 0), MARGIN * bar.repeat_interleave(t, 0) + TINY


SIM_SIZES = [1, 63, 64, 65, 130]
SIM_D = [16, 768]
SIM_SCALES = [1.0, 1000.0]


def sim_operands(family, n, m, d, seed):
    g = G.gen(seed)
    if family == 'exact':
        return torch.randint(-4, 5, (n, d), generator=g).float(), torch.randint(-8, 9, (m, d), generator=g).float()
    return torch.randn(n, d, generator=g), torch.randn(m, d, generator=g) * torch.exp2(torch.randint(-3, 4, (m, 1), generator=g).float())


def sim_emulate(a, b, scale, rows_alloc, ldo, mutate=None):
    """The whole (rows_alloc, ldo) output buffer of an fp32 emulation on top of the canary.  mutate 'write_past_n': a ragged tile row written past n."""
    n, m = a.shape[0], b.shape[0]
    buf = G.canary((rows_alloc, ldo), torch.float32)
    buf[:n, :m] = (a.float() @ b.float().t()) * _f32(scale)
    if mutate == 'write_past_n':
        buf[n, :m] = 0.0
    return buf


def sim_verdict(family, a, b, scale, got, prefill, stats=None):
    """got / prefill: the whole (rows_alloc, ldo) fp32 buffer.  exact: integer sums below 2^24 times the scale, one rounding -> bit for bit.  wide: d fused or unfused
    additions in sequence (similarity_f32_kernel, sf_clip.hip) + the scale's product: (d + 1) 2^-24 scale sum |a b|."""
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    sc = _f32(scale)
    ref, T = (a.double() @ b.double().t()) * sc, (a.double().abs() @ b.double().abs().t()) * sc
    if family == 'exact':
        assert float(T.max()) / sc < 2 ** 24
        mm = G.exact_mismatch(got[:n, :m], ref, False)
        msgs = [f'similarity: {mm}'] if mm else []
    else:
        msgs = within(got[:n, :m], ref, (d + 1) * U32 * T, 'similarity', stats, 'similarity')
    written = torch.zeros_like(got, dtype=torch.bool)
    written[:n, :m] = True
    return msgs + damage(got, prefill, written, 'similarity')


SHIFT_CASES = [(14, 8), (14, 14), (32, 1), (33, 2), (5, 3)]


def shift_seed(S, W):
    """The seed of a case's blocks: one at which every case's predictions tell the corruptions of the CPU screen apart (asserted there for every case; at S = 5 a
    block is small enough for some seeds to give W - 1 terms the same argmax)."""
    return S * 7 + W + 3


def shift_operands(n_clips, S, W, ldg, seed):
    """G (n_clips * S, ldg) fp32.  Every clip's diagonal block is its own random integer matrix in [-8, 8] (asymmetric; every window sum exact in fp32), so the
    predictions depend on the data, on W, on the clip and on the direction of the argmax.  Ties are planted INTO that block, n = S - W + 1 >= 3: the windows (0, 1),
    (0, n - 1) and (n - 1, n - 1) are filled with 8 - each sums to 8 W, the largest possible value, so row 0 holds its maximum at columns 1 and n - 1 and column
    n - 1 at rows 0 and n - 1, and the first one must win (n = 2: the windows (0, 0), (0, 1) and (1, 1)).  Everything outside the diagonal blocks is 1e30."""
    g = G.gen(seed)
    n = S - W + 1
    Gm = torch.full((n_clips * S, ldg), 1e30)
    w = torch.arange(W)
    for b in range(n_clips):
        blk = torch.randint(-8, 9, (S, S), generator=g).float()
        wins = [(0, 1), (0, n - 1), (n - 1, n - 1)] if n >= 3 else [(0, 0), (0, 1), (1, 1)] if n == 2 else []
        for i, j in wins:
            blk[i + w, j + w] = 8.0
        Gm[b * S:(b + 1) * S, b * S:(b + 1) * S] = blk
    return Gm


def shift_reference(Gm, n_clips, S, W, mutate=None):
    """Explicit-loop float64 restatement of shift_and_get_preds on the similarity matrix: sim[i][j] = sum_w G[i + w][j + w] inside a clip's block,
    preds_a[j] = argmax_i, preds_v[i] = argmax_j, the first maximum winning (torch.argmax).  mutate (the corruptions): 'last' - the last maximum wins;
    'short_window' - windows of W - 1 terms; 'next_clip' - the block of the next clip is read."""
    n = S - W + 1
    pa, pv = torch.zeros(n_clips, n, dtype=torch.int64), torch.zeros(n_clips, n, dtype=torch.int64)
    better = (lambda a, b: a >= b) if mutate == 'last' else (lambda a, b: a > b)
    terms = W - 1 if mutate == 'short_window' else W
    for b in range(n_clips):
        c = (b + 1) % n_clips if mutate == 'next_clip' else b
        blk = Gm[c * S:(c + 1) * S, c * S:(c + 1) * S].double().tolist()
        sim = [[sum(blk[i + w][j + w] for w in range(terms)) for j in range(n)] for i in range(n)]
        for j in range(n):
            best = 0
            for i in range(1, n):
                if better(sim[i][j], sim[best][j]):
                    best = i
            pa[b, j] = best
        for i in range(n):
            best = 0
            for j in range(1, n):
                if better(sim[i][j], sim[i][best]):
                    best = j
            pv[b, i] = best
    return pa, pv


def shift_verdict(Gm, n_clips, S, W, got_a, got_v):
    pa, pv = shift_reference(Gm, n_clips, S, W)
    msgs = []
    for name, got, ref in (('preds_a', got_a, pa), ('preds_v', got_v, pv)):
        if not torch.equal(got, ref):
            i = (got != ref).nonzero()[0].tolist()
            msgs.append(f'{name}: {int((got != ref).sum())} of {ref.numel()} differ, first at {i}: got {int(got[tuple(i)])} want {int(ref[tuple(i)])}')
    return msgs


RG_G = [1, 7, 8, 16, 17, 196]
RG_COLS = [8, 64, 520]
RG_NSEQ = [1, 3]


def reduce_groups_is_vec(G_, cols, strides_aligned):
    """sf_reduce_groups_bf16 (sf_towerbwd.hip): the vector kernel needs cols % 8 == 0, G >= 8, every stride % 8 == 0 and 16-byte aligned pointers."""
    return cols % 8 == 0 and G_ >= 8 and strides_aligned


def reduce_groups_depth(G_, vec, accumulate):
    """vector kernel: ceil(G / 16) groups per slice in sequence, then the 15 other slices added in sequence; scalar kernel: G in sequence; + the accumulate add."""
    return (-(-G_ // 16) + 15 if vec else G_) + int(accumulate)


def reduce_groups_emulate(x, prefill, accumulate, mutate=None):
    """x (n_seq, G, cols) bf16, prefill (n_seq, cols) bf16 -> bf16.  mutate 'missing_last_group'."""
    xs = x[:, :-1] if mutate == 'missing_last_group' else x
    acc = xs.float().sum(1)
    if accumulate:
        acc = acc + prefill.float()
    return acc.bfloat16()


def reduce_groups_verdict(x, prefill, accumulate, vec, got, stats=None):
    xd = x.double()
    ref, T = xd.sum(1), xd.abs().sum(1)
    if accumulate:
        ref, T = ref + prefill.double(), T + prefill.double().abs()
    return within(got.float(), ref, G.bf16_ulp(ref) / 2 + (reduce_groups_depth(x.shape[1], vec, accumulate) + 1) * U32 * T, 'reduce_groups', stats, 'reduce_groups')
