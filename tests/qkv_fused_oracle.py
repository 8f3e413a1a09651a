"""Host-side oracle of the fused "qkv projection + divided attention" tests (tests/test_qkv_fused_gpu.py, tests/test_qkv_fused_oracle_cpu.py): operand families, the
float64 reference computed from the raw operands X, W, bias, side / qkv_cls and key_keep, the emulation, the bars and the mutations of the screen.  Nothing here touches
a GPU API; every function works on the device its tensors live on (the larger cases run it on the device in float64, as the GEMM tile-walk tests do).

Operation.  qkv = bf16(X W^T + bias) for every row the kernel projects (all three kernels round the projection to bf16 before the attention: sf_qkv_space.hip "Epilogue:
accumulators (+ bias) -> bf16 -> LDS", sf_qkv_time2.hip "Epilogue (1)", sf_qkv_time.hip "the accumulators are rounded to bf16 first"); the rows it does not project - the
CLS row and tokens 192 .. 195 of every frame (`side`, 33 rows per sequence) for sf_qkv_space_attention / sf_qkv_time_attention2, the CLS row (`qkv_cls`) for
sf_qkv_time_attention - are taken as given.  Then grouped_attention_fwd_ref of tests/test_attention_fwd_gpu.py (imported, not copied): space groups = [CLS key; the
frame's 196 tokens], time groups = [CLS key; the patch's 8 frames], keys with key_keep == 0 removed.  The CLS query's softmax state is laid out in the records each kernel
documents (record_rows): space 8 per (sequence, head), record f = frame f, the CLS key in record 0; time2 33, record 4 tb + j = patches 24 tb + 6 j .. + 5 (three 16-row
key tiles of the patch-major arrays) in their 8 frames, record 32 = patches 192 .. 195 and the CLS key; round 3 n_groups / 4, record r = patches 4 r .. 4 r + 3, the CLS
key in record 0.  The CLS key is counted in exactly one record.

Families.
  exact  gemm_oracle's `sparse` operands times powers of two.  bf16: X rows hold at most 16 entries +-2^-2 in columns 0 .. 703, W integers in [-8, 8] times 2^-(e - 2),
         bias integers in [-64, 64] times 2^-e with e chosen per block of output features (q | k | v): every sum is at most 16 * 8 + 64 = 192 units of 2^-e - a bf16
         number -, and every fp32 partial sum an integer number of units below 2^24: exact in any order.  MXFP8: at most 12 bytes +-1 per row with scale bytes
         125 .. 127, W bytes 0 / +-1 with scale bytes (129 - e) .. (131 - e): |x w| <= 16 units, every sum at most 12 * 16 + 64 = 256.  (The issue's 126 .. 128 become
         these so that q and k land at sigma ~ 0.5; the spread of three consecutive scale bytes per 32-block is kept.)  assert_exact checks both properties on the host
         before anything runs.  The in-kernel bf16 rounding is then the identity and q | k | v are known exactly, so the kernel is held to the attention bars.
           flat      e = 6 for q | k | v: q, k sigma 42 units = 0.66.
           marked    flat + marks: columns 704 .. 767 of X are indicator columns, weighted 0 in every row of W but the marks'.  A row's indicator (value 16 units of X)
                     sits at column 704 + j, j = (t + 6 f) % 48 for token t of frame f (at most five tokens of a frame share one; the 8 frames of a patch differ),
                     48 + i for side token 192 + i, 52 for the CLS row, 53 for the rows behind the last sequence; W row (v, head h, column c_j) holds 8 at column 704 + j,
                     c_j = 8 + j (j < 48), 56 + i, 60, 61: v of that row carries +128 units = 2.0 there.  The other v weights are 0 / +-1, the v bias integers in
                     [-8, 8] (noise sigma ~ 6 units): 16 + 8 + 128 <= 255.  A dropped, doubled or foreign key moves an output by 128 p units; at p ~ 1 / 197 that
                     is 0.65 units against a bar of about 0.03.  The marks come from X, W and bias (and side, which is the projection of marked rows): nothing is edited
                     after the projection.
           sharp     marked with e_q = 0 (q sigma 42): scores span about +-30.
           negative  k bias c, q bias -c with |c| in 40 .. 60 units, q | k weights in [-2, 2], v = 1 + noise: every real score is about -5, a zero-filled key slot that
                     leaks (score 0) outweighs the real keys.
           uniform   marked with W_q = 0, no q bias and +32 units on the v bias (v > 0): every score is exactly 0 in any arithmetic, the exponentials are exactly 1 and their bf16 packing is the identity
                     - the input on which the bf16 output is known bit for bit (MXFP8 output form).
         side_differs: the X rows of the side tokens and of the CLS row are replaced by other rows' content AFTER `side` was made: a kernel that projects them from X
         reads other marks.
  wide   gemm_oracle.operands / mx_operands('wide') with W (the W scale bytes) times one power of two that brings rms(q) to about 1 (a property of the inputs).

Bars (stated before any measurement).  exact: the attention bars of test_attention_fwd_gpu.py - sf_qkv_space.hip and sf_qkv_time2.hip copy attn_mfma_kernel (P packed to
bf16: A = sum_k p_k |v_kd|), sf_qkv_time.hip copies attn_tiny64_kernel (fp32 to the store: A = 0).  No header documents a further rounding.  A record's m carries
2^-126 on top of its bar, so that a record whose scores are all exactly 0 (`uniform`: bar 0, error 0) compares as 0 <= 2^-126 and not as 0 / 0.
wide: the reference rounds its float64 projection to bf16; the kernel rounds its fp32 projection.  Per projected element dq = u |q| + F_gemm,
F_gemm = (gemm_oracle.depth(768, mfma) + 1) 2^-24 (sum_k |x_k w_k| + |bias|) with mfma = '32x32x16' (bf16 forms of all three kernels) or '32x32x64' (MX forms, plus
gemm_oracle.mx_group_term); dq = 0 for the given rows.  (A bf16 value that flips to its neighbour moves by one ulp <= 2 u |q|, u |q| more than dq charges it, on that
element alone; dq charges u |q| to all 64 elements of a dot product, of which fewer than 1 % can flip.)  Through the scores: ds_ik = scale sum_d (dq_id |k_kd| +
|q_id| dk_kd + dq_id dk_kd); through the softmax: p'_k / p_k = e^(d_k) / sum_l p_l e^(d_l) with |d| <= ds, so |p'_k - p_k| <= p_k expm1(ds_ik + max_l ds_il) =: p_k r_ik;
through P V: P_id = sum_k p_k r_ik |v_kd| + sum_k p_k (1 + r_ik) dv_kd.  bar = MARGIN (u (A + |ref|) + F + P).  Records at the reference maximum: l within
sum_k e_k expm1(ds_k), o within sum_k e_k (expm1(ds_k) |v_kd| + e^(ds_k) dv_kd), m within log2(e) max_k ds_k, on top of their attention bars.
Statistical, per (sequence, head, row kind): ||got - ref||_2 <= STAT_FACTOR ||emu - ref||_2 + ||F||_2, emu = gemm_oracle.emulate (32-deep k-blocks in fp32, bf16) followed
by the attention emulation (P packed where the kernel packs), F = the attention's fp32 term + the propagation of F_gemm alone.  MARGIN = 1.5, STAT_FACTOR = 2.0."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as GO  # noqa: E402
import test_attention_fwd_gpu as AF  # noqa: E402

U, U32, MARGIN, STAT_FACTOR, LOG2E = AF.U, AF.U32, AF.MARGIN, AF.STAT_FACTOR, AF.LOG2E
N_TOK, FRAMES, HEADS, HD, DM = 196, 8, 12, 64, 768
SCALE = 0.125
EXACT_FAMILIES = ('flat', 'marked', 'sharp', 'negative', 'uniform')
IND0 = 704                      # first indicator column of X
PACKS_P = {'space': True, 'time2': True, 'time': False}
GROUPING = {'space': 'space', 'time2': 'time', 'time': 'time'}
MFMA = {'bf16': '32x32x16', 'mx': '32x32x64'}


def seq_rows(G=N_TOK):
    return 1 + FRAMES * G


def side_index(n_seq):
    """Row ids of [the CLS row; tokens 192 .. 195 of each of the 8 frames] per sequence, 33 per sequence, in the order of `side`."""
    seq = torch.arange(n_seq).view(n_seq, 1) * seq_rows()
    left = 1 + torch.arange(FRAMES).view(FRAMES, 1) * N_TOK + 192 + torch.arange(4).view(1, 4)
    return torch.cat([seq, seq + left.reshape(1, 32)], 1).reshape(-1)


def cls_index(n_seq, G):
    return torch.arange(n_seq) * seq_rows(G)


def geometry(grouping, G=N_TOK):
    """(n_groups, row0, group_stride, tok_stride, n_tok, cls_row) of grouped_attention_fwd_ref."""
    return (FRAMES, 1, G, 1, G, 0) if grouping == 'space' else (G, 1, 1, G, FRAMES, 0)


def record_rows(layout, G=N_TOK):
    """(P, Kmax) rows (within a sequence) of the keys of each CLS-query record of one kernel, -1 = padding."""
    fr = torch.arange(FRAMES)
    if layout == 'space':
        rows = torch.full((FRAMES, G + 1), -1, dtype=torch.int64)
        rows[:, :G] = 1 + fr[:, None] * G + torch.arange(G)[None]
        rows[0, G] = 0
        return rows
    if layout == 'time2':
        assert G == N_TOK
        rows = torch.full((33, 48), -1, dtype=torch.int64)
        for r in range(32):
            p = 24 * (r // 4) + 6 * (r % 4) + torch.arange(6)
            rows[r] = (1 + fr[None] * G + p[:, None]).flatten()
        rows[32, :32] = (1 + fr[None] * G + (192 + torch.arange(4))[:, None]).flatten()
        rows[32, 32] = 0
        return rows
    assert layout == 'time' and G % 4 == 0
    rows = torch.full((G // 4, 33), -1, dtype=torch.int64)
    for r in range(G // 4):
        rows[r, :32] = (1 + fr[None] * G + (4 * r + torch.arange(4))[:, None]).flatten()
    rows[0, 32] = 0
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operand families
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _indicators(n_seq, G, extra):
    """Per row of X (n_seq * seq_rows + extra): the indicator index j (module docstring)."""
    R = seq_rows(G)
    r = torch.arange(n_seq * R + extra)
    s = r % R
    f, t = (s - 1).clamp_min(0) // G, (s - 1).clamp_min(0) % G
    j = (t + 6 * f) % 48
    if G == N_TOK:
        j = torch.where(t >= 192, 48 + (t - 192), j)
    j = torch.where(s == 0, torch.full_like(j, 52), j)
    j[n_seq * R:] = 53
    return j


def _mark_col(j):
    return torch.where(j < 48, 8 + j, torch.where(j < 52, 56 + (j - 48), 8 + j))       # 52 -> 60, 53 -> 61


def _e4m3(v):
    return int(torch.tensor(float(v)).to(torch.float8_e4m3fn).view(torch.uint8))


def exact_operands(kind, n_seq, family, seed, G=N_TOK, side_differs=False, bias=True, extra=2):
    """One `exact` case (module docstring).  Returns dict(kind, family, n_seq, G, x (rows + extra, 768) float64 = what the kernel reads, x_given (the rows `side` /
    `qkv_cls` are the projection of, indexed like x), w (2304, 768) float64, bias (2304,) float64 or None, unit (2304,) float64; bf16: xb, wb bf16; mx: xq, xsc, wq, wsc)."""
    assert family in EXACT_FAMILIES and kind in ('bf16', 'mx')
    R = seq_rows(G)
    rows = n_seq * R
    marks = family in ('marked', 'sharp', 'uniform')
    e = torch.full((3,), 6, dtype=torch.int64)                                     # the unit 2^-e of q | k | v
    if family == 'sharp':
        e[0] = 0
    j = _indicators(n_seq, G, extra)
    mark_rows = (2 * DM + torch.arange(HEADS)[:, None] * HD + _mark_col(torch.arange(54))[None]).flatten()   # (12 * 54,) rows of W
    mark_cols = (IND0 + torch.arange(54))[None].expand(HEADS, 54).flatten()
    if kind == 'bf16':
        o = GO.operands('sparse', rows + extra, 3 * DM, DM, seed, a_rows=rows + extra)
        xi, wi, bi = o['a'].double(), o['w'].double(), o['bias'].double()
        xi[:, IND0:], wi[:, IND0:] = 0.0, 0.0
        if marks:
            xi[torch.arange(rows + extra), IND0 + j] = 16.0
            wi[mark_rows, mark_cols] = 8.0
    else:
        o = GO.mx_operands('sparse', rows + extra, 3 * DM, DM, seed)
        xq, xsc, wq, wsc, bi = o['aq'].clone(), o['asc'].clone(), o['wq'].clone(), o['wsc'].clone(), o['bias'].double()
        xq[:, IND0:], wq[:, IND0:] = 0, 0
        xsc[:, IND0 // 32:], wsc[:, IND0 // 32:] = 128, 128
        if marks:
            xq[torch.arange(rows + extra), IND0 + j] = _e4m3(1.0)
            wq[mark_rows, mark_cols] = _e4m3(8.0)
    small_v = marks or family == 'negative'
    small_qk = family == 'negative'
    if kind == 'bf16':
        shrink = lambda w_: torch.sign(w_) * (w_.abs() > 4)                        # noqa: E731  integers in [-8, 8] -> 0 / +-1
        if small_v:
            wi[2 * DM:, :IND0] = shrink(wi[2 * DM:, :IND0])
        if small_qk:
            wi[:2 * DM, :IND0] = torch.div(wi[:2 * DM, :IND0], 4, rounding_mode='trunc')
    else:
        nb = IND0 // 32
        if small_v:
            wsc[2 * DM:, :nb] = wsc[2 * DM:, :nb].clamp(max=127)
        if small_qk:
            wsc[:2 * DM, :nb] = wsc[:2 * DM, :nb].clamp(max=127)
    if marks:
        bi[2 * DM:] = torch.div(bi[2 * DM:], 8, rounding_mode='trunc')
    if family == 'negative':
        c = torch.where(bi[DM:2 * DM] < 0, -1.0, 1.0) * (40 + bi[DM:2 * DM].abs() % 21)
        bi[:DM], bi[DM:2 * DM], bi[2 * DM:] = -c, c, 64.0
    if family == 'uniform':
        bi[:DM] = 0.0
        bi[2 * DM:] += 32.0                                                         # v > 0: |o| = sum p |v|, the fp32 term stays far below an ulp of the output (88 + 8 + 32 + 128 = 256)
        if kind == 'bf16':
            wi[:DM] = 0.0
        else:
            wq[:DM] = 0
    unit = torch.exp2(-e.double()).repeat_interleave(DM)
    out = dict(kind=kind, family=family, n_seq=n_seq, G=G, exact=True, unit=unit, bias=(bi * unit) if bias else None)
    if kind == 'bf16':
        x = xi * 0.25
        w = wi * (unit * 4.0)[:, None]
        out.update(xb=x.bfloat16(), wb=w.bfloat16())
        assert torch.equal(out['xb'].double(), x) and torch.equal(out['wb'].double(), w)
    else:
        xsc = (xsc.int() - 1).to(torch.uint8)                                       # 126 .. 128 -> 125 .. 127: X in units of 2^-2
        wsc = (wsc.int() + (3 - e.repeat_interleave(DM).int())[:, None]).to(torch.uint8)   # 126 .. 128 -> (129 - e) .. (131 - e)
        x, w = GO.mx_dequant(xq, xsc), GO.mx_dequant(wq, wsc)
        out.update(xq=xq, xsc=xsc, wq=wq, wsc=wsc)
    out['x_given'] = x.clone()
    if side_differs:                                                               # the kernel must not read these rows of X: give them another row's content
        idx = side_index(n_seq) if G == N_TOK else cls_index(n_seq, G)
        src = (idx + 5) % rows
        x[idx] = x[src]
        if kind == 'bf16':
            out['xb'][idx] = out['xb'][src]
        else:
            out['xq'][idx], out['xsc'][idx] = out['xq'][src], out['xsc'][src]
    out.update(x=x, w=w)
    return out


def wide_operands(kind, n_seq, seed, G=N_TOK, bias=True, extra=2):
    """One `wide` case: gemm_oracle's wide family, W times the power of two that brings rms(q) to about 1."""
    rows = n_seq * seq_rows(G)
    if kind == 'bf16':
        o = GO.operands('wide', rows + extra, 3 * DM, DM, seed, a_rows=rows + extra)
        x, w = o['a'].double(), o['w'].double()
    else:
        o = GO.mx_operands('wide', rows + extra, 3 * DM, DM, seed)
        x, w = o['a'], o['w']
    b = o['bias'].double() * 0.25
    rms = (x[:256] @ w[:DM].t()).pow(2).mean().sqrt().item()
    sh = int(round(math.log2(rms)))
    out = dict(kind=kind, family='wide', n_seq=n_seq, G=G, exact=False, bias=b if bias else None)
    if kind == 'bf16':
        w = w * 2.0 ** -sh
        out.update(xb=x.bfloat16(), wb=w.bfloat16())
        assert torch.equal(out['wb'].double(), w)
    else:
        wsc = (o['wsc'].int() - sh).clamp(1, 254).to(torch.uint8)
        w = GO.mx_dequant(o['wq'], wsc)
        out.update(xq=o['aq'], xsc=o['asc'], wq=o['wq'], wsc=wsc)
    out.update(x=x, w=w, x_given=x)
    return out


def assert_exact(ops, proj, S):
    """The two properties of the `exact` family: every projected element is a bf16 number, and every partial sum is an integer number of units below 2^24."""
    unit = ops['unit'].to(proj.device)
    n = proj / unit
    assert torch.equal(n, n.round()), 'exact family: a projection is not a whole number of units'
    assert (S / unit).max().item() < 2.0 ** 24, 'exact family: a partial sum may leave the fp32 integers'
    assert torch.equal(AF._rb(proj), proj), f'exact family: {int((AF._rb(proj) != proj).sum())} projected elements are not bf16 numbers (max {n.abs().max().item()} units)'


def project(ops, device='cpu', x_key='x'):
    """float64 projection of every row of ops[x_key] (without the rows behind the last sequence) and S = sum |x w| + |bias|."""
    rows = ops['n_seq'] * seq_rows(ops['G'])
    x, w = ops[x_key][:rows].to(device), ops['w'].to(device)
    b = ops['bias'].to(device) if ops['bias'] is not None else None
    return GO.reference(x, w, b)


def given_rows(ops, which):
    """(index, values): the rows the kernel takes as given - `side` (n_seq * 33, 2304) or `qkv_cls` (n_seq, 2304) - as bf16, made on the host by rounding the float64
    projection of x_given."""
    idx = side_index(ops['n_seq']) if which == 'side' else cls_index(ops['n_seq'], ops['G'])
    b = ops['bias'] if ops['bias'] is not None else None
    pre, _ = GO.reference(ops['x_given'][idx], ops['w'], b)
    return idx, pre.float().bfloat16()


def qkv_values(ops, which, device='cpu', from_x=False):
    """What the attention of the kernel must see: (qkv (rows, 2304) float64 = bf16(float64 projection) with the given rows put in, dq = the wide family's per-element
    projection error or None).  from_x: mutation 10 - the given rows recomputed from X."""
    proj, S = project(ops, device)
    if ops['exact']:
        assert_exact(ops, proj, S)
    qkv = AF._rb(proj)
    idx, given = given_rows(ops, which)
    if not from_x:
        qkv[idx] = given.double().to(device)
    dq = None
    if not ops['exact']:
        F = (GO.depth(DM, MFMA[ops['kind']]) + 1) * U32 * S
        if ops['kind'] == 'mx':
            rows = ops['n_seq'] * seq_rows(ops['G'])
            F = F + GO.mx_group_term(ops['x'][:rows].to(device), ops['w'].to(device))
        dq = dict(full=U * qkv.abs() + F, fp32=F)
        for d in dq.values():
            d[idx] = 0.0
    return qkv, dq


def emulated_qkv(ops, which, device='cpu', kblocks=None):
    """gemm_oracle.emulate of the projection (32-deep k-blocks in fp32, bias, bf16) with the given rows put in.  kblocks: mutation 8."""
    rows = ops['n_seq'] * seq_rows(ops['G'])
    b = ops['bias'].to(device) if ops['bias'] is not None else None
    emu = GO.emulate(ops['x'][:rows].to(device), ops['w'].to(device), b, None, gelu=False, out_bf16=True, kblocks=kblocks).double()
    idx, given = given_rows(ops, which)
    emu[idx] = given.double().to(device)
    return emu


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def split_heads(qkv, n_seq, G, heads=None):
    x = qkv.view(n_seq, seq_rows(G), 3, HEADS, HD)
    if heads is not None:
        x = x[:, :, :, heads]
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def _gather_records(q, k, v, keep, rows):
    n, R, H, D = q.shape
    P, Km = rows.shape
    rc = rows.clamp_min(0)
    K = k[:, rc].permute(0, 1, 3, 2, 4)                                            # (n, P, H, Km, D)
    V = v[:, rc].permute(0, 1, 3, 2, 4)
    M = keep[:, rc] & (rows >= 0).to(keep.device)                                  # (n, P, Km)
    Q = q[:, 0][:, None, :, None, :].expand(n, P, H, 1, D)
    return Q, K, V, M[:, :, None, None, :]


def cls_records(q, k, v, keep, rows, packs_p):
    """The CLS query's records in a kernel's layout (`rows` of record_rows), shaped as the 'rec' of grouped_attention_fwd_ref: (n, H, P) and (n, H, P, D)."""
    D = q.shape[-1]
    c = AF._attend(*_gather_records(q, k, v, keep, rows), SCALE, packs_p)
    hg = lambda x: x[:, :, :, 0].transpose(1, 2)                                    # noqa: E731
    empty = hg(c['dead'])
    return dict(m=torch.where(empty, torch.full_like(hg(c['mx']), -math.inf), hg(c['mx']) * LOG2E), l=hg(c['l']), o=hg(c['eV']), empty=empty,
                mbar=MARGIN * (D + 2) * U32 * LOG2E * hg(c['sabs_max']) + AF.TINY, lbar=MARGIN * hg(c['Fl']), obar=MARGIN * (U * hg(c['eA']) + hg(c['Fo'])))


def merge_records(m, l, o):
    """float64 merge of records (n, H, P) / (n, H, P, D): the row and (M, L)."""
    M = m.amax(-1)
    w = torch.exp2(m - M[..., None])
    L = (l * w).sum(-1)
    return (o * w[..., None]).sum(2) / L[..., None], M, L


def _propagate(Q, K, V, dQ, dK, dV, mask):
    """First-order-and-a-half propagation of the projection's error (module docstring).  Shapes as AF._attend.  Returns P (.., Tq, D) for the normalised output and
    (dl, do, dm) for the un-normalised state at the reference maximum."""
    s = SCALE * (Q @ K.mT)
    ds = SCALE * (dQ @ K.abs().mT + Q.abs() @ dK.mT + dQ @ dK.mT)
    mask = mask.expand(s.shape)
    ds = torch.where(mask, ds, torch.zeros_like(ds))
    sm = torch.where(mask, s, torch.full_like(s, -math.inf))
    dead = ~mask.any(-1, keepdim=True)
    mx = torch.where(dead, torch.zeros_like(s[..., :1]), sm.amax(-1, keepdim=True))
    e = torch.exp(sm - mx)
    p = torch.nan_to_num(e / e.sum(-1, keepdim=True))
    r = torch.expm1(ds + ds.amax(-1, keepdim=True))
    P = (p * r) @ V.abs() + (p * (1 + r)) @ dV
    r1 = torch.expm1(ds)
    return P, (e * r1).sum(-1), (e * r1) @ V.abs() + (e * (1 + r1)) @ dV, LOG2E * ds.amax(-1)


def _grp(x, idx):
    return x[:, idx].permute(0, 1, 3, 2, 4)


def propagated(q, k, v, dq, dk, dv, geo, keep, rows):
    """The propagation terms of one case: 'tok' (n, G, H, T, D), 'row' (n, H, D), 'rec' dict(l, o, m) in the record layout."""
    n, R, H, D = q.shape
    G, row0, gs, ts, T, cls_row = geo
    idx = row0 + torch.arange(G)[:, None] * gs + torch.arange(T)[None] * ts
    cat = lambda x: torch.cat([x[:, cls_row][:, None, :, None, :].expand(n, G, H, 1, D), _grp(x, idx)], 3)   # noqa: E731
    Mg = torch.cat([keep[:, cls_row][:, None, None].expand(n, G, 1), keep[:, idx]], 2)[:, :, None, None, :]
    tok = _propagate(_grp(q, idx), cat(k), cat(v), _grp(dq, idx), cat(dk), cat(dv), Mg)[0]
    allr = torch.arange(R)[None]
    one = lambda x: x[:, 0][:, None, :, None, :]                                     # noqa: E731
    row, rl, _, rm = _propagate(one(q), _grp(k, allr), _grp(v, allr), one(dq), _grp(dk, allr), _grp(dv, allr), keep[:, None, None, None, :])
    row, rl, rm = row[:, 0, :, 0], rl[:, 0, :, 0], rm[:, 0, :, 0]
    Q, K, V, M = _gather_records(q, k, v, keep, rows)
    dQ, dK, dV, _ = _gather_records(dq, dk, dv, keep, rows)
    _, dl, do, dm = _propagate(Q, K, V, dQ, dK, dV, M)
    hg = lambda x: x[:, :, :, 0].transpose(1, 2)                                      # noqa: E731
    return dict(tok=tok, row=row, L=rl, M=rm, rec=dict(l=hg(dl), o=hg(do), m=hg(dm)))


def fused_reference(qkv, n_seq, G, layout, keep=None, dq=None, emu_qkv=None, heads=None):
    """The float64 reference of one fused launch from the values of qkv_values(): grouped_attention_fwd_ref's dict ('tok', 'row', 'M', 'L', ..) with 'rec' in the
    kernel's record layout and 'P' = n_part.  dq (wide family): the propagated terms are added to the bars and to F; emu_qkv: the emulation's projection (else the
    emulation runs on qkv itself)."""
    dev = qkv.device
    q, k, v = split_heads(qkv, n_seq, G, heads)
    geo = geometry(GROUPING[layout], G)
    rows = record_rows(layout, G)
    packs = PACKS_P[layout]
    kp = torch.ones(n_seq, seq_rows(G), dtype=torch.bool, device=dev) if keep is None else keep.to(dev).bool().view(n_seq, seq_rows(G))
    ref = AF.grouped_attention_fwd_ref(q, k, v, geo, SCALE, kp, packs_p=packs, cls_query=True, combine_parts=rows.shape[0])
    ref['rec'] = cls_records(q, k, v, kp, rows, packs)
    ref['P'] = rows.shape[0]
    ref['Mbar'] = ref['Mbar'] + AF.TINY                                              # (as the records' m: 0 <= 2^-126 where every score is exactly 0)
    if emu_qkv is not None:
        e = AF.grouped_attention_fwd_ref(*split_heads(emu_qkv, n_seq, G, heads), geo, SCALE, kp, packs_p=packs, cls_query=True, combine_parts=rows.shape[0])
        ref['tok'].emu, ref['row'].emu = e['tok'].emu, e['row'].emu
    if dq is not None:
        full = propagated(q, k, v, *split_heads(dq['full'], n_seq, G, heads), geo, kp, rows)
        fp32 = propagated(q, k, v, *split_heads(dq['fp32'], n_seq, G, heads), geo, kp, rows)
        for kind in ('tok', 'row'):
            ref[kind].bar = ref[kind].bar + MARGIN * full[kind]
            ref[kind].F = ref[kind].F + fp32[kind]
        ref['Mbar'], ref['Lbar'] = ref['Mbar'] + MARGIN * full['M'], ref['Lbar'] + MARGIN * full['L']
        rec = ref['rec']
        rec['lbar'] = rec['lbar'] + MARGIN * torch.nan_to_num(full['rec']['l'])
        rec['obar'] = rec['obar'] + MARGIN * torch.nan_to_num(full['rec']['o'])
        rec['mbar'] = rec['mbar'] + MARGIN * torch.nan_to_num(full['rec']['m'])
    return ref


def tokens_of(out, n_seq, G, layout, heads=HEADS):
    """(rows, >= 768) output values -> (n, groups, H, T, D) as the 'tok' section is shaped."""
    geo = geometry(GROUPING[layout], G)
    idx = geo[1] + torch.arange(geo[0])[:, None] * geo[2] + torch.arange(geo[4])[None] * geo[3]
    got = out.view(n_seq, seq_rows(G), -1)[..., :heads * HD].reshape(n_seq, seq_rows(G), heads, HD)
    return got[:, idx].permute(0, 1, 3, 2, 4)


def rows_of(tok, n_seq, G, layout):
    """The inverse of tokens_of for the patch rows: (n, groups, H, T, D) -> (n, seq_rows, H, D) with the CLS row zero."""
    geo = geometry(GROUPING[layout], G)
    idx = geo[1] + torch.arange(geo[0])[:, None] * geo[2] + torch.arange(geo[4])[None] * geo[3]
    out = torch.zeros(n_seq, seq_rows(G), tok.shape[2], tok.shape[4], dtype=tok.dtype, device=tok.device)
    out[:, idx] = tok.permute(0, 1, 3, 2, 4)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------------------------------
MASKS = ('random20', 'random80', 'frame', 'patch', 'side', 'seam191', 'seam192', 'last', 'ones')


def key_keep(pattern, n_seq, seed=0, G=N_TOK):
    """(n_seq, seq_rows) bool key flags of one pattern; the CLS flag is always 1."""
    R = seq_rows(G)
    keep = torch.ones(n_seq, R, dtype=torch.bool)
    tok = keep[:, 1:].view(n_seq, FRAMES, G)                                        # a view: edits land in keep
    g = GO.gen(1000 + seed)
    if pattern in ('random20', 'random80'):
        tok &= torch.rand(n_seq, FRAMES, G, generator=g) >= (0.2 if pattern == 'random20' else 0.8)
    elif pattern == 'frame':
        tok[n_seq - 1, 3] = False                                                  # a CLS record without a key (space), m = -inf, l = 0
        tok[0, 0, ::3] = False
    elif pattern == 'patch':
        tok[0, :, min(50, G - 1)] = False                                          # a time group whose only key is the CLS key
        tok[n_seq - 1, :, G - 1] = False
    elif pattern == 'side':
        tok[:, :, max(G - 4, 0):] = False
    elif pattern == 'seam191':
        tok[:, :, min(191, G - 1)] = False
    elif pattern == 'seam192':
        tok[:, :, min(192, G - 1)] = False
    elif pattern == 'last':
        tok[n_seq - 1, FRAMES - 1, G - 1] = False
    else:
        assert pattern == 'ones'
    return keep


# ---------------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, sec):
    """Worst |got - ref| / bar over a section (inf for a NaN)."""
    r = (got - sec.ref).abs() / sec.bar
    return torch.nan_to_num(r, nan=float('inf')).max().item()


def stat_ratio(got, sec):
    """Worst ||got - ref|| / (STAT_FACTOR ||emu - ref|| + ||F||) per (sequence, head)."""
    dims = (1, 3, 4) if got.dim() == 5 else (2,)
    l2 = lambda x: (x * x).sum(dims).sqrt()                                         # noqa: E731
    return torch.nan_to_num(l2(got - sec.ref) / (STAT_FACTOR * l2(sec.emu - sec.ref) + l2(sec.F)), nan=float('inf')).max().item()


def record_ratios(part, rec):
    """part (n, H, P, 66) float64 against the reference records, rescaled to the reference maximum: worst ratios (m, l, o)."""
    m, l, o = part[..., 0], part[..., 1], part[..., 2:]
    live = ~rec['empty']
    dm = torch.where(live, m - rec['m'], torch.zeros_like(m))
    f = torch.exp2(dm)
    mx = lambda r: torch.nan_to_num(r[live], nan=float('inf')).max().item() if live.any() else 0.0   # noqa: E731
    return mx(dm.abs() / rec['mbar']), mx((l * f - rec['l']).abs() / rec['lbar']), mx((o * f[..., None] - rec['o']).abs() / rec['obar'])


def known_bf16(ref, err):
    """Elements whose bf16 rounding is the same over [ref - err, ref + err]: there the kernel's bf16 output is known bit for bit (rounding is monotone)."""
    return AF._rb(ref - err) == AF._rb(ref + err)


def preround_error(sec, packing_exact=False):
    """The bound on the kernel's fp32 result in front of its bf16 store: the bar without the store's own rounding.  packing_exact (`uniform` family: every exponential
    is exactly 1, a bf16 number): the P-packing term u A is not there either, only the fp32 term is left."""
    return MARGIN * sec.F if packing_exact else sec.bar - MARGIN * U * sec.ref.abs()


def mx_expected(ref_rows, err_rows):
    """Host MXFP8 quantisation (gemm_oracle.mx_quant_ref, the restatement of _mx_quant_ref) of the reference's bf16 output rows (rows, 768) float64, and where it is
    known: a block's scale byte where the block's largest magnitude has the same exponent at both ends of its interval, an element's byte where its bf16 value is known
    (known_bf16) and its block's scale is.  Returns bytes (rows, 768), scale bytes (rows, 24), element mask (rows, 768), scale mask (rows, 24)."""
    q, sc = GO.mx_quant_ref(ref_rows.float().bfloat16().cpu())
    lo, hi = AF._rb(ref_rows - err_rows).abs(), AF._rb(ref_rows + err_rows).abs()
    blk = lambda x: x.view(x.shape[0], -1, 32).amax(-1).clamp_min(2.0 ** -126)      # noqa: E731
    sk = torch.floor(torch.log2(blk(torch.minimum(lo, hi)))) == torch.floor(torch.log2(blk(torch.maximum(lo, hi))))
    ek = known_bf16(ref_rows, err_rows) & sk.repeat_interleave(32, 1)
    return q, sc, ek.cpu(), sk.cpu()
