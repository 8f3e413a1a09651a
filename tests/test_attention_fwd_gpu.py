"""GPU: the forward attention kernels of csrc/sf_attention.hip (attn_mfma_kernel<D, NKT>, attn_tiny64_kernel<PART>, attn_cls64_kernel, attn_cls_combine64[_mx]_kernel)
element by element against a float64 restatement of the same operation, computed on the host from the very bf16-rounded inputs the kernel sees, at the tile, mask and
argument edges of the launchers.  Conventions as in test_attention_bwd_gpu.py.

Reference (grouped_attention_fwd_ref): s = scale q k^T, p = softmax(s) over [CLS key; the group's tokens] minus the keys with keep == 0, o = p v, with the group
geometry of the ABI; for the CLS query the per-group softmax records, the merged row and (M, L).  It is checked once against torch.softmax in float64 on keys gathered
by explicit loops (test_reference_matches_float64_softmax, no GPU).

Bars.  u = 2^-8 (bf16), e = 2^-24 (fp32).  For every written bf16 element  |got - ref| <= 1.5 * (u * (A + |ref|) + F), where
  A  = sum_k p_k |v_kd| for attn_mfma_kernel (it packs the un-normalised exponentials to bf16 before the P V MFMA) and 0 for attn_tiny64_kernel and attn_cls64_kernel,
     which are fp32 up to the store;  u |ref| is the bf16 rounding of the output itself;
  F  is the fp32 term: the score's head_dim-term dot and the exponent's argument as a relative error of p (ds_k = e ((head_dim + 2) scale sum_d |q_d k_kd| + 2 |s_k|),
     own score and the largest ds of the row for the maximum's), the normaliser ((nk + 8) e), (nk + 16) e A-like absolute sums, and 2^-126 sum_k |v_kd| where v_exp_f32
     flushes.  attn_cls64_kernel rescales its accumulator once per key step (online softmax, __expf): chain depth ceil(n_keys / 32) + 8 in place of 8, and the rescale
     factors' arguments telescope to at most the score range, so the maximum's ds counts twice.
CLS partial records (fp32, not unique in m) are compared as l 2^(m - m_ref), o[d] 2^(m - m_ref) against (l_ref, o_ref) at the reference maximum under
1.5 (u A_rec + F_rec), A_rec = sum_k e_k |v_kd| (MFMA kernel; l is summed before the packing: no u term) or 0 (tiny kernel); m within 1.5 (head_dim + 2) e log2(e) scale
max_k sum_d |q_d k_kd| of m_ref; statistics (M, L) likewise, L relative (n + 16) e plus the score term.
sf_attention_cls_combine: one bf16 rounding plus (n_part + 8) e of the absolute sums, plus - stated before any measurement - (|m_i - M| + 2) e per weight: the argument of
exp2(m_i - M) is one fp32 subtraction of numbers up to 100, whose rounding is a relative error ln 2 e |m_i - M| / 2 of the weight.
Statistical criterion per (sequence, head, row kind) with >= 64 elements: ||got - ref||_2 <= 2 ||emu - ref||_2 + ||F||_2, emu rounding to bf16 where the kernel does.

Inputs (Gaussian, rounded to bf16, scale head_dim^-0.5): 'flat' (q sigma 0.25: every p within a small factor of 1 / nk), 'marked' (flat + v of token t carries +64 in
column 8 + t % 48 of every head - at most five tokens of a group share a column, so a column's bar stays far below one token's share -, the CLS key in column 60,
and every row outside the groups holds k = 0, v = 128: a dropped, doubled or leaked key moves an output by 64 p ~ 0.3; a leaked zero-filled slot (k = v = 0) only
rescales the row by 1 - 1 / nk, about 64 / nk^2 - invisible at large nk, hence the negative family), 'sharp' (q sigma 10: scores span +-30; marked v with sigma 0.25 noise, so that the marked columns read single probabilities with a relative bar of about 1 %),
'negative' (keys share a component c, queries are -c + noise: every score is about -5, v = 1 + noise - a zero-filled key slot that leaks (score 0) outweighs the real keys).
Every comparison covers all written elements; outputs are pre-filled with a position-dependent bf16 canary and must be bit-equal wherever the kernel must not write.
Rows whose query has no kept key at all are 0 / 0 in the reference too: exactly those rows are left out, in the two dedicated cases of test_masked_dead_group.

Measured on an MI355X (319 tests, 15 s; worst error / bar, worst rel-L2 / limit): attn_mfma_kernel<64> 0.57, 0.50 (masked 0.57, 0.50; with the CLS query 0.58, 0.50; records
m 0.016, l 0.006, o 0.59); attn_mfma_kernel<96> 0.55, 0.50 (masked 0.55, 0.49); attn_tiny64_kernel 0.66, 0.50 (masked 0.66, 0.50; records m 0.015, l 0.007, o 0.012);
attn_cls64_kernel 0.65, 0.50 (masked 0.65, 0.50; M 0.015, L 0.005); attn_cls_combine64_kernel 0.66, 0.50 on both paths (L 0.05 / 0.02); partial + combine 0.65, 0.62
(M 0.014, L 0.005).  0.66 = 1 / 1.5 is an output that sits half a bf16 ulp from the reference: the fp32 kernels are at the floor of their bars.  No bar needed an
addition after the measurement."""
import math

import pytest
import torch

U = 2.0 ** -8             # bf16 unit roundoff of the bars
U32 = 2.0 ** -24          # fp32 unit roundoff
TINY = 2.0 ** -126        # v_exp_f32 flushes results below the smallest normal
MARGIN = 1.5              # second-order terms and v_exp_f32, once on the whole bar
STAT_FACTOR = 2.0
LOG2E = 1.4426950408889634
BF = torch.bfloat16
FAMILIES = ('flat', 'marked', 'sharp', 'negative')


def _lib():
    from synchformer_amd import _lib as L
    return L.load()


def _ops():
    from synchformer_amd import ops
    return ops


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from synchformer_amd import _lib as L
    L.check(rc, what)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rb(x):
    """float64 -> nearest bf16 -> float64 (the emulation's rounding points)."""
    return x.to(torch.float32).to(BF).to(torch.float64)


def _canary(rows, cols, seed=0):
    """Finite bf16 values in [2, 4) whose bits depend on the position: a kernel that skips a store, or stores where it must not, is seen bit for bit."""
    i = torch.arange(rows * cols, dtype=torch.int64) * 37 + seed
    return (0x4000 + (i % 128)).to(torch.int16).view(rows, cols).view(BF)


def _assert_untouched(got, canary, written, what):
    bad = (got.view(torch.int16) != canary.view(torch.int16)) & ~written
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} elements outside the written set changed, first at row {i[0]} column {i[1]}')


def _unravel(flat, shape):
    out = []
    for dim in reversed(shape):
        out.append(flat % dim)
        flat //= dim
    return out[::-1]


def _rejected(rc, what):
    assert rc == -1, f'{what}: expected -1, got {rc}'
    assert _lib().sf_last_error().decode(errors='replace').strip(), f'{what}: no message'


# ======================================================================================================================================
# Reference
# ======================================================================================================================================
class _Sec:
    """One row kind: exact float64 result, element bar, emulation and fp32 term, all shaped alike ((n, G, H, T, D) for token rows, (n, H, D) for CLS rows)."""

    def __init__(self, ref, bar, emu, F):
        self.ref, self.bar, self.emu, self.F = ref, bar, emu, F


def _direct(ref, A, F, emu):
    """A row that the kernel stores itself: one bf16 rounding of its fp32 accumulator."""
    return _Sec(ref, MARGIN * (U * (A + ref.abs()) + F), _rb(emu), F)


def _attend(Q, K, V, mask, scale, packs_p, depth=8, chain=False):
    """Independent attention problems.  Q (..., Tq, D), K, V (..., nk, D) float64, mask (..., 1 | Tq, nk) bool (False: the key is removed).  Returns the exact output o, the
    absolute sum A = sum_k p_k |v_kd| (zero unless packs_p), the fp32 term F, the emulation (before the output rounding), `dead` (queries without a kept key: 0 / 0), and the
    un-normalised state at the exact maximum: mx (natural domain), l = sum_k e_k, eV = sum_k e_k v_k, eA = sum_k e_k |v_k|, with their fp32 terms Fl, Fo."""
    D, nk = Q.shape[-1], K.shape[-2]
    s = scale * (Q @ K.mT)
    sabs = scale * (Q.abs() @ K.abs().mT)
    mask = mask.expand(s.shape)
    sm = torch.where(mask, s, torch.full_like(s, -math.inf))
    dead = ~mask.any(-1)
    mx = torch.where(dead, torch.zeros_like(s[..., 0]), sm.amax(-1))
    e = torch.exp(sm - mx[..., None])                                              # exactly 0 at removed keys
    l = e.sum(-1, keepdim=True)
    aV = V.abs()
    ds = torch.where(mask, U32 * ((D + 2) * sabs + 2 * s.abs()), torch.zeros_like(s))   # absolute error of a score = relative error of its exponential
    rel = ds + (2 if chain else 1) * ds.amax(-1, keepdim=True)                     # own score and the maximum's
    p = e / l                                                                     # NaN where dead
    o, A = p @ V, p @ aV
    flush = TINY * aV.sum(-2, keepdim=True)
    F = (p * (rel + (nk + depth) * U32)) @ aV + (nk + depth + 8) * U32 * A + flush
    eV, eA = e @ V, e @ aV
    emu = (_rb(e) @ V) / l if packs_p else o
    return dict(o=o, A=A if packs_p else torch.zeros_like(A), F=F, emu=emu, dead=dead, mx=mx, l=l[..., 0], eV=eV, eA=eA if packs_p else torch.zeros_like(eA),
                Fscore=(e * rel).sum(-1), Fl=(e * rel).sum(-1) + (nk + depth) * U32 * l[..., 0], Fo=(e * rel) @ aV + (nk + depth + 8) * U32 * eA + flush,
                sabs_max=torch.where(mask, sabs, torch.zeros_like(s)).amax(-1), p=p, rel=rel)


def _stats_bars(r, D, n_keys, depth=16):
    """(M, L) of one query in the base-2 domain with their bars, from _attend's state: M within the fp32 error of the largest score, L relative (n + depth) e + score term."""
    M = torch.where(r['dead'], torch.full_like(r['mx'], -math.inf), r['mx'] * LOG2E)
    Mbar = MARGIN * (D + 2) * U32 * LOG2E * r['sabs_max']
    Lbar = MARGIN * (r['Fscore'] + (n_keys + depth) * U32 * r['l'])
    return M, r['l'], Mbar, Lbar


def grouped_attention_fwd_ref(q, k, v, geometry, scale, keep=None, packs_p=True, cls_query=False, combine_parts=0):
    """float64 forward of the grouped attention of sf_attention: q, k, v (n_seq, seq_rows, heads, D) float64 (the bf16 inputs, widened);
    geometry = (n_groups, row0, group_stride, tok_stride, n_tok, cls_row).  Token t of group g is row row0 + g group_stride + t tok_stride and attends
    [row cls_row (if >= 0); its group's tokens]; keep (n_seq, seq_rows), 0 = that row is removed as a key for every query and for the CLS query (its own output is still
    computed).  packs_p: the kernel packs its exponentials to bf16 before P V (attn_mfma_kernel) or not (attn_tiny64_kernel).
    Returns 'tok' (_Sec, (n, G, H, T, D)), 'dead' (n, G): groups whose queries have no kept key, 'idx' (G, T); with cls_query the CLS query (row cls_row, attends every
    kept key of the sequence, the CLS key once) as 'rec': per (n, H, G) the record at the reference maximum - m (base 2), l, o (.., D), their bars and `empty` -, 'row'
    (_Sec, (n, H, D)) for partial + combine over combine_parts records, and 'M', 'L', 'Mbar', 'Lbar' (n, H) in the base-2 domain."""
    n, R, H, D = q.shape
    G, row0, gs, ts, T, cls_row = geometry
    has_cls = cls_row >= 0
    idx = row0 + torch.arange(G)[:, None] * gs + torch.arange(T)[None] * ts
    kp = torch.ones(n, R, dtype=torch.bool) if keep is None else keep.bool()

    def grp(x):
        return x[:, idx].permute(0, 1, 3, 2, 4)                                   # (n, G, H, T, D)

    Qg, Kg, Vg, Mg = grp(q), grp(k), grp(v), kp[:, idx]                            # Mg (n, G, T)
    if has_cls:
        Kg = torch.cat([k[:, cls_row][:, None, :, None, :].expand(n, G, H, 1, D), Kg], 3)
        Vg = torch.cat([v[:, cls_row][:, None, :, None, :].expand(n, G, H, 1, D), Vg], 3)
        Mg = torch.cat([kp[:, cls_row][:, None, None].expand(n, G, 1), Mg], 2)
    r = _attend(Qg, Kg, Vg, Mg[:, :, None, None, :], scale, packs_p)
    out = {'idx': idx, 'tok': _direct(r['o'], r['A'], r['F'], r['emu']), 'dead': r['dead'][:, :, 0, 0]}
    if cls_query:
        assert has_cls
        nk = T + 1
        qc = q[:, cls_row]                                                         # (n, H, D)
        Mc = Mg.clone()
        Mc[:, 1:, 0] = False                                                       # the CLS key counts for the CLS query in group 0 only
        c = _attend(qc[:, None, :, None, :].expand(n, G, H, 1, D), Kg, Vg, Mc[:, :, None, None, :], scale, packs_p)
        hg = lambda x: x[:, :, :, 0].transpose(1, 2)                                # noqa: E731  (n, G, H, 1, ...) -> (n, H, G, ...)
        empty = hg(c['dead'])
        out['rec'] = dict(m=torch.where(empty, torch.full_like(hg(c['mx']), -math.inf), hg(c['mx']) * LOG2E), l=hg(c['l']), o=hg(c['eV']), empty=empty,
                          mbar=MARGIN * (D + 2) * U32 * LOG2E * hg(c['sabs_max']), lbar=MARGIN * hg(c['Fl']), obar=MARGIN * (U * hg(c['eA']) + hg(c['Fo'])))
        Kall = torch.cat([k[:, cls_row][:, :, None], grp(k).permute(0, 2, 1, 3, 4).reshape(n, H, G * T, D)], 2)
        Vall = torch.cat([v[:, cls_row][:, :, None], grp(v).permute(0, 2, 1, 3, 4).reshape(n, H, G * T, D)], 2)
        Mall = torch.cat([kp[:, cls_row][:, None], kp[:, idx.flatten()]], 1)       # (n, 1 + G T)
        a = _attend(qc[:, :, None, :], Kall, Vall, Mall[:, None, None, :], scale, packs_p, depth=8 + combine_parts + 8)
        out['row'] = _direct(a['o'][:, :, 0], a['A'][:, :, 0], a['F'][:, :, 0], a['emu'][:, :, 0])
        out['row_dead'] = a['dead'][:, :, 0]
        a1 = {key: (val[:, :, 0] if val.dim() >= 3 else val) for key, val in a.items()}
        out['M'], out['L'], out['Mbar'], out['Lbar'] = _stats_bars(a1, D, 1 + G * T, depth=16 + combine_parts)
        assert nk == Kg.shape[3]
    return out


def _geometry(G, T, layout, cls, extra=2):
    """layout 'contig' (tok_stride 1, group_stride n_tok), 'time' (group_stride 1, tok_stride n_groups) or 'single' (one group, row0 = 0, group_stride 0); cls 'none',
    'first' (row 0, tokens from row 1) or 'last' (the row behind the groups, tokens from row 0).  Without a CLS row the groups start at row 1 (row 0 is foreign)."""
    if layout == 'single':
        G, gs, ts = 1, 0, 1
        cls = 'last' if cls == 'first' else cls
    elif layout == 'contig':
        gs, ts = T, 1
    else:
        gs, ts = 1, G
    span = (G - 1) * gs + (T - 1) * ts + 1
    if cls == 'first':
        cls_row, row0 = 0, 1
    elif cls == 'last':
        cls_row, row0 = span, 0
    else:
        cls_row, row0 = -1, (0 if layout == 'single' else 1)
    return (G, row0, gs, ts, T, cls_row), max(row0 + span, cls_row + 1) + extra


def _inputs(n, R, geo, H, D, family, seed, ld):
    """The packed q | k | v buffer (n * R, ld) bf16 of one input family (module docstring)."""
    G, row0, gs, ts, T, cls_row = geo
    Hd = H * D
    g = _gen(seed)
    x = torch.randn(n, R, ld, generator=g)
    q, k, v = x[..., :Hd], x[..., Hd:2 * Hd], x[..., 2 * Hd:3 * Hd]
    if family in ('flat', 'marked'):
        q *= 0.25
    elif family == 'sharp':
        q *= 10.0
        v *= 0.25
    elif family == 'negative':
        c = torch.randn(Hd, generator=g) * 0.8
        k.mul_(0.3).add_(c)
        q.sub_(c)
        v += 1.0
    else:
        assert family == 'plain'
    if family in ('marked', 'sharp'):
        idx = row0 + torch.arange(G)[:, None] * gs + torch.arange(T)[None] * ts
        heads = torch.arange(H) * D
        other = torch.ones(R, dtype=torch.bool)
        other[idx.flatten()] = False
        for t in range(T):
            v[:, idx[:, t][:, None], (heads + 8 + t % 48)[None]] += 64.0
        if cls_row >= 0:
            other[cls_row] = False
            v[:, cls_row, heads + 60] += 64.0
        v[:, other] = 128.0                                                        # rows no group owns: a read past the group is seen
        k[:, other] = 0.0
    return x.view(n * R, ld).to(BF)


def _softmax_loops(q, k, v, geo, scale, keep, cls_query):
    """The same forward written independently (python loops over groups, torch.softmax with -inf masks)."""
    n, R, H, D = q.shape
    G, row0, gs, ts, T, cls_row = geo
    rows = {}
    for g in range(G):
        tok = [row0 + g * gs + t * ts for t in range(T)]
        keys = ([cls_row] if cls_row >= 0 else []) + tok
        s = scale * torch.einsum('nthd,nkhd->nhtk', q[:, tok], k[:, keys])
        if keep is not None:
            s = s.masked_fill(~keep.bool()[:, keys][:, None, None, :], -math.inf)
        o = torch.einsum('nhtk,nkhd->nthd', torch.softmax(s, -1), v[:, keys])
        for j, r in enumerate(tok):
            rows[r] = o[:, j]
    lse2 = None
    if cls_query:
        keys = [cls_row] + [row0 + g * gs + t * ts for g in range(G) for t in range(T)]
        s = scale * torch.einsum('nhd,nkhd->nhk', q[:, cls_row], k[:, keys])
        if keep is not None:
            s = s.masked_fill(~keep.bool()[:, keys][:, None, :], -math.inf)
        rows[cls_row] = torch.einsum('nhk,nkhd->nhd', torch.softmax(s, -1), v[:, keys])
        lse2 = torch.logsumexp(s, -1) * LOG2E
    zero = torch.zeros(n, H, D, dtype=torch.float64)
    return torch.stack([rows.get(r, zero) for r in range(R)], 1), lse2


@pytest.mark.parametrize('G,T,layout,cls,D,masked', [(3, 5, 'contig', 'first', 64, False), (3, 5, 'time', 'first', 64, True), (2, 20, 'time', 'last', 64, True),
                                                      (2, 7, 'contig', 'none', 96, True), (1, 9, 'single', 'none', 96, False)])
def test_reference_matches_float64_softmax(G, T, layout, cls, D, masked):
    """CPU: grouped_attention_fwd_ref (batched over groups, explicit exponentials) equals torch.softmax in float64 on keys gathered by loops, with -inf masks and in the
    strided time layout, to 1e-12; its CLS records merge to its CLS row and to (M, L); the emulation stays within the element bars, which are positive."""
    geo, R = _geometry(G, T, layout, cls)
    n, H = 2, 3
    x = _inputs(n, R, geo, H, D, 'plain', 5, 3 * H * D).double().view(n, R, 3, H, D)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    keep = None
    if masked:
        keep = (torch.rand(n, R, generator=_gen(1)) > 0.4)
        keep[:, geo[1]] = True                                                    # one kept key per group 0 ...
        keep[:, geo[1] + geo[2]] = True                                           # ... and group 1: no dead group here
        if geo[0] > 2:
            keep[:, geo[1] + 2 * geo[2]] = True
        keep[1, geo[1] + geo[3]] = False
    clsq = geo[5] >= 0
    ref = grouped_attention_fwd_ref(q, k, v, geo, D ** -0.5, keep, cls_query=clsq)
    want, lse2 = _softmax_loops(q, k, v, geo, D ** -0.5, keep, clsq)
    assert not ref['dead'].any()
    got = torch.zeros_like(want)
    got[:, ref['idx']] = ref['tok'].ref.permute(0, 1, 3, 2, 4)
    if clsq:
        got[:, geo[5]] = ref['row'].ref
        rec = ref['rec']
        w = torch.exp2(rec['m'] - ref['M'][..., None])
        L = (rec['l'] * w).sum(-1)
        assert ((rec['o'] * w[..., None]).sum(2) / L[..., None] - ref['row'].ref).abs().max() <= 1e-12
        assert (L - ref['L']).abs().max() <= 1e-12 * L.max()
        assert (ref['M'] + torch.log2(ref['L']) - lse2).abs().max() <= 1e-12 * lse2.abs().max().clamp_min(1.0)
    assert (got - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
    for sec in [ref['tok']] + ([ref['row']] if clsq else []):
        assert ((sec.emu - sec.ref).abs() <= sec.bar).all() and (sec.bar > 0).all()


@pytest.mark.parametrize('D', [64, 96])
def test_reference_distinguishes_marked_inputs(D):
    """CPU: at the largest group (nk = 208, p ~ 1 / 208) the reference alone tells a dropped key (marked family: the last token removed) and a leaked zero-filled key slot
    (negative family: one more key with k = v = 0) from the truth by more than 10 bars - so the element bars cannot hide either."""
    n, H, T = 1, 2, 207
    geo, R = _geometry(2, T, 'contig', 'first')
    for family, worst_needed in (('marked', 10.0), ('sharp', 10.0), ('negative', 10.0)):
        x = _inputs(n, R, geo, H, D, family, 3, 3 * H * D).double().view(n, R, 3, H, D)
        q, k, v = x[:, :, 0].clone(), x[:, :, 1].clone(), x[:, :, 2].clone()
        ref = grouped_attention_fwd_ref(q, k, v, geo, D ** -0.5)
        if family == 'negative':                                                  # a leaked slot: the row behind each group's last token becomes an extra zero key
            geo2, R2 = _geometry(2, T + 1, 'contig', 'first')
            q2, k2, v2 = [torch.zeros(n, R2, H, D, dtype=torch.float64) for _ in range(3)]
            for g in range(2):
                src = slice(1 + g * T, 1 + (g + 1) * T)
                dst = slice(1 + g * (T + 1), 1 + g * (T + 1) + T)
                q2[:, dst], k2[:, dst], v2[:, dst] = q[:, src], k[:, src], v[:, src]
            q2[:, 0], k2[:, 0], v2[:, 0] = q[:, 0], k[:, 0], v[:, 0]
            bad = grouped_attention_fwd_ref(q2, k2, v2, geo2, D ** -0.5)['tok'].ref[:, :, :, :T]
        else:                                                                     # a dropped key: the last token of every group
            keep = torch.ones(n, R, dtype=torch.bool)
            keep[:, ref['idx'][:, -1]] = False
            bad = grouped_attention_fwd_ref(q, k, v, geo, D ** -0.5, keep)['tok'].ref
        ratio = ((bad - ref['tok'].ref).abs() / ref['tok'].bar).max().item()
        assert ratio > worst_needed, (family, ratio)


# ======================================================================================================================================
# Comparison
# ======================================================================================================================================
WORST = {}                 # kernel -> worst observed error / bar ratio (printed per test, collected by the report at the end of the module)
EXCLUDED = set()           # the cases that left rows without any kept key out of the numeric comparison (at most two, test_masked_dead_group)


def _worst(name, value):
    WORST[name] = max(WORST.get(name, 0.0), value if math.isfinite(value) else float('inf'))


def _check_section(kernel, kind, got, sec, key_shift=0, stat=True):
    """Element bar over every element of the section, then the statistical criterion per (sequence, head).  Returns the worst error / bar ratio."""
    err = (got - sec.ref).abs()
    ratio = err / sec.bar
    worst = ratio.max().item() if ratio.numel() else 0.0
    _worst(kernel, worst)
    bad = ~(err <= sec.bar)
    if bad.any():
        flat = torch.where(bad, torch.nan_to_num(ratio, nan=float('inf')), torch.zeros_like(ratio)).flatten().argmax().item()
        i = _unravel(flat, ratio.shape)
        if got.dim() == 5:
            where = f'sequence {i[0]} group {i[1]} head {i[2]} row {i[3]} (tile {(i[3] + key_shift) // 16}) dim {i[4]}'
        else:
            where = f'sequence {i[0]} head {i[1]} dim {i[2]}'
        raise AssertionError(f'{kernel} {kind}: {int(bad.sum())} of {bad.numel()} elements outside the bar; worst at {where}: got {got[tuple(i)].item()!r} '
                             f'want {sec.ref[tuple(i)].item()!r} bar {sec.bar[tuple(i)].item()!r} (err / bar = {ratio[tuple(i)].item():.3g})')
    worst_stat = 0.0
    if stat:
        dims = (1, 3, 4) if got.dim() == 5 else (2,)
        per = got[0].numel() // got.shape[2 if got.dim() == 5 else 1]
        if per >= 64:
            l2 = lambda x: (x * x).sum(dims).sqrt()                                   # noqa: E731
            e, thr = l2(got - sec.ref), STAT_FACTOR * l2(sec.emu - sec.ref) + l2(sec.F)
            r = e / thr
            worst_stat = r.max().item()
            _worst(kernel + ' (rel-L2 / limit)', worst_stat)
            if not (e <= thr).all():
                s_, h_ = _unravel(torch.nan_to_num(r, nan=float('inf')).flatten().argmax().item(), r.shape)
                nrm = l2(sec.ref)[s_, h_].item()
                raise AssertionError(f'{kernel} {kind}: sequence {s_} head {h_}: rel-L2 error {e[s_, h_].item() / max(nrm, 1e-300):.3g} above '
                                     f'{thr[s_, h_].item() / max(nrm, 1e-300):.3g} = 2 x the bf16 emulation\'s distance (+ fp32 term); ratio {r[s_, h_].item():.3g}, '
                                     f'worst element err / bar {worst:.3g}')
    return worst, worst_stat


def _check_records(kernel, part, rec):
    """part (n, H, G, 66) float64 from the kernel against the reference records (grouped_attention_fwd_ref 'rec')."""
    assert not torch.isnan(part).any(), f'{kernel}: NaN in a CLS record'
    m, l, o = part[..., 0], part[..., 1], part[..., 2:]
    empty = rec['empty']
    assert (l[empty] == 0).all() and (o[empty] == 0).all(), f'{kernel}: the record of a group without a kept key is not merge-neutral (l, o must be 0)'
    live = ~empty
    assert torch.isfinite(part[live]).all(), f'{kernel}: non-finite CLS record'
    dm = torch.where(live, m - rec['m'], torch.zeros_like(m))
    f = torch.exp2(dm)
    rm = (dm.abs() / rec['mbar'])[live]
    rl = ((l * f - rec['l']).abs() / rec['lbar'])[live]
    ro = ((o * f[..., None] - rec['o']).abs() / rec['obar'])[live]
    for name, r in (('m', rm), ('l', rl), ('o', ro)):
        w = r.max().item() if r.numel() else 0.0
        _worst(f'{kernel} record {name}', w)
        assert w <= 1.0, f'{kernel}: CLS record {name} outside its bar: worst err / bar {w:.3g}'


def _check_stats(kernel, st, ref):
    """st (n, H, 2) float64 = (M, L) from the kernel against the reference's base-2 statistics."""
    assert torch.isfinite(st).all(), f'{kernel}: statistics not finite'
    dm = st[..., 0] - ref['M']
    rm = (dm.abs() / ref['Mbar']).max().item()
    rl = ((st[..., 1] * torch.exp2(dm) - ref['L']).abs() / ref['Lbar']).max().item()
    _worst(kernel + ' statistics M', rm)
    _worst(kernel + ' statistics L', rl)
    assert rm <= 1.0 and rl <= 1.0, f'{kernel}: statistics outside their bars: M {rm:.3g}, L {rl:.3g}'


class _Run:
    """Host and device buffers of one grouped-attention forward: q | k | v are column blocks of one packed (rows, ld) buffer, the output a canary-filled (rows, ldo) buffer;
    pad widens ld / ldo beyond 3 * heads * D / heads * D (multiples of 8)."""

    def __init__(self, gpu, n, G, H, D, T, layout='contig', cls='first', family='flat', seed=0, pad=(0, 0), extra=2):
        self.geo, self.R = _geometry(G, T, layout, cls, extra)
        self.n, self.G, self.H, self.D, self.T, self.Hd = n, self.geo[0], H, D, T, H * D
        self.cls_row = self.geo[5]
        self.ld, self.ldo = 3 * self.Hd + pad[0], self.Hd + pad[1]
        self.qkv_h = _inputs(n, self.R, self.geo, H, D, family, 100 + seed, self.ld)
        self.qkv = self.qkv_h.to(gpu)
        self.canary = _canary(n * self.R, self.ldo, seed)
        self.gpu, self.scale = gpu, D ** -0.5
        G_, row0, gs, ts, _, _ = self.geo
        self.idx = row0 + torch.arange(G_)[:, None] * gs + torch.arange(T)[None] * ts
        self.packs_p = not (D == 64 and T <= 8)                                    # attn_mfma_kernel or attn_tiny64_kernel

    def views(self):
        Hd = self.Hd
        return self.qkv[:, :Hd], self.qkv[:, Hd:2 * Hd], self.qkv[:, 2 * Hd:3 * Hd]

    def kw(self):
        G, row0, gs, ts, T, cls_row = self.geo
        return dict(n_seq=self.n, seq_rows=self.R, n_groups=G, row0=row0, group_stride=gs, tok_stride=ts, n_tok=T, cls_row=cls_row, heads=self.H, head_dim=self.D,
                    scale=self.scale)

    def wide(self):
        x = self.qkv_h.double().view(self.n, self.R, self.ld)[..., :3 * self.Hd].reshape(self.n, self.R, 3, self.H, self.D)
        return x[:, :, 0], x[:, :, 1], x[:, :, 2]

    def keep_dev(self, keep):
        return None if keep is None else keep.to(torch.uint8).contiguous().view(-1).to(self.gpu)

    def attention(self, keep=None):
        out = self.canary.clone().to(self.gpu)
        _ops().attention(*self.views(), out, key_keep=self.keep_dev(keep), **self.kw())
        return out

    def partial(self, keep=None):
        out = self.canary.clone().to(self.gpu)
        part = torch.full((self.n * self.H * self.G * 66,), float('nan'), device=self.gpu)
        _ops().attention_cls_partial(*self.views(), out, part, key_keep=self.keep_dev(keep), **self.kw())
        return out, part

    def ref(self, keep=None, cls_query=False):
        return grouped_attention_fwd_ref(*self.wide(), self.geo, self.scale, keep, packs_p=self.packs_p, cls_query=cls_query, combine_parts=self.G if cls_query else 0)

    def tokens(self, raw):
        got = raw.double().view(self.n, self.R, self.ldo)[..., :self.Hd].reshape(self.n, self.R, self.H, self.D)
        return got[:, self.idx].permute(0, 1, 3, 2, 4)

    def check_tokens(self, kernel, out, ref, case=None, cls_written=False):
        """Every token row against its bar, everything else against the canary.  `case`: the name of a dedicated dead-group case (rows without a kept key)."""
        torch.cuda.synchronize()
        raw = out.cpu()
        got, sec, dead = self.tokens(raw), ref['tok'], ref['dead']
        if case is None:
            assert not dead.any(), 'a group without any kept key outside the dedicated cases'
            assert torch.isfinite(got).all(), f'{kernel}: non-finite output'
        else:
            assert int(dead.sum()) == 1, 'a dedicated case holds exactly one group without a kept key'
            EXCLUDED.add(case)
            assert len(EXCLUDED) <= 2, f'rows are left out of the comparison in more than two cases: {sorted(EXCLUDED)}'
            live = ~dead[:, :, None, None, None].expand_as(got)
            assert (torch.isfinite(got) | ~live).all(), f'{kernel}: a row with a kept key is not finite'
            z, one = torch.zeros_like(got), torch.ones_like(got)
            got = torch.where(live, got, z)
            sec = _Sec(torch.where(live, sec.ref, z), torch.where(live, sec.bar, one), torch.where(live, sec.emu, z), torch.where(live, sec.F, z))
        res = _check_section(kernel, 'token rows', got, sec, key_shift=1 if self.cls_row >= 0 else 0)
        written = torch.zeros(self.n, self.R, self.ldo, dtype=torch.bool)
        written[:, self.idx.flatten(), :self.Hd] = True
        if cls_written:
            written[:, self.cls_row, :self.Hd] = True
        _assert_untouched(raw, self.canary, written.view(self.n * self.R, self.ldo), kernel)
        return res

    def cls_row_of(self, out):
        return out.cpu().double().view(self.n, self.R, self.ldo)[:, self.cls_row, :self.Hd].reshape(self.n, self.H, self.D)


def _kernel_name(run):
    return 'attn_tiny64_kernel' if not run.packs_p else f'attn_mfma_kernel<{run.D}>'


def _run_attention(gpu, **kw):
    run = _Run(gpu, **kw)
    return run.check_tokens(_kernel_name(run), run.attention(), run.ref())


# ======================================================================================================================================
# 1. sf_attention, attn_mfma_kernel<D, NKT>: every instantiation
# ======================================================================================================================================
def _nks(D, nkt):
    if D == 64 and nkt == 1:
        return [10, 12, 15, 16]                                                     # n_tok > 8 keeps D = 64 on the MFMA path
    return [16 * (nkt - 1) + 1, 16 * (nkt - 1) + 8, 16 * nkt - 1, 16 * nkt]


@pytest.mark.gpu
@pytest.mark.parametrize('nkt', range(1, 14))
@pytest.mark.parametrize('D', [64, 96])
def test_mfma_every_instantiation(gpu, D, nkt):
    """attn_mfma_kernel<D, NKT> at nk = n_tok + has_cls = 16 (NKT - 1) + 1, a middle value, 16 NKT - 1 and 16 NKT, each with and without a CLS key (row 0 or the last row),
    rotating over the contiguous, the time and the single-group layout and padded strides; every shape on the marked and the negative family and on flat or sharp in turn.
    Rounding points: exponentials packed to bf16 before P V (A = sum_k p_k |v_kd|), bf16 store.  Checks the unrolled last-tile mask, the zero half of the odd last pair
    of the P V loop, K_IT staging and MAXQ query tiles of each instantiation."""
    i = 0
    for nk in _nks(D, nkt):
        for cls in ('none', 'first' if nk % 2 else 'last'):
            T = max(nk - (0 if cls == 'none' else 1), 1)
            layout = ('contig', 'time', 'single')[i % 3]
            for family in ('marked', 'negative', 'flat' if i % 2 else 'sharp'):
                _run_attention(gpu, n=2, G=2, H=3, D=D, T=T, layout=layout, cls=cls, family=family, seed=nk * 7 + i, pad=(8, 16) if i % 2 else (0, 0))
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [
    dict(n=1, G=8, H=12, D=64, T=196, layout='contig', cls='first'),               # Motionformer space attention
    dict(n=2, G=1, H=12, D=64, T=74, layout='single', cls='none'),                 # AST
    dict(n=2, G=1, H=8, D=96, T=184, layout='single', cls='none'),                 # syncability
    dict(n=2, G=1, H=8, D=96, T=198, layout='single', cls='none'),                 # sync transformer
    dict(n=2, G=1, H=12, D=64, T=197, layout='single', cls='none'),
    dict(n=2, G=1, H=12, D=64, T=13, layout='single', cls='none'),
    dict(n=2, G=1, H=12, D=64, T=17, layout='single', cls='none'),
], ids=lambda kw: f"G{kw['G']}-T{kw['T']}-D{kw['D']}-H{kw['H']}")
@pytest.mark.parametrize('family', ['marked', 'sharp'])
def test_mfma_product_shapes(gpu, kw, family):
    """The shapes the model runs, with their head counts."""
    _run_attention(gpu, family=family, seed=3, pad=(8, 8), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [96])
@pytest.mark.parametrize('T', range(1, 9))
def test_mfma_d96_small_groups(gpu, D, T):
    """head_dim 96 has no tiny kernel: n_tok 1 .. 8 run attn_mfma_kernel<96, 1>."""
    for cls in ('none', 'first'):
        for family in ('marked', 'negative'):
            _run_attention(gpu, n=2, G=3, H=3, D=D, T=T, layout='time', cls=cls, family=family, seed=T)


@pytest.mark.gpu
def test_mfma_query_tile_rotation(gpu):
    """3 sequences x 8 groups x 12 heads = 288 workgroups at NKT 13 with 13 query tiles (n_tok 207 + CLS): the rotation wq = (wave + xw + (xw >> 5)) & 3 takes all four
    values, xw >> 5 is non-zero from workgroup 256 on, and one wave owns four query tiles.  Compared in full."""
    _run_attention(gpu, n=3, G=8, H=12, D=64, T=207, layout='contig', cls='first', family='marked', seed=1)
    _run_attention(gpu, n=3, G=8, H=12, D=64, T=207, layout='time', cls='first', family='negative', seed=2, pad=(8, 8))


# ======================================================================================================================================
# 2. sf_attention, attn_tiny64_kernel<false>
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('T', range(1, 9))
@pytest.mark.parametrize('cls', ['none', 'first', 'last'])
def test_tiny_every_n_tok(gpu, T, cls):
    """attn_tiny64_kernel<false> is fp32 up to its store: A = 0, bar = 1.5 (u |ref| + F).  Idle query lanes (n_tok < 8) shadow the last token and the key slots beyond nk
    re-read key nk - 1 with s = -inf: a marked last key that counted twice would be seen.  units = n_seq n_groups heads = 1, 3, 4, 5 (four waves per workgroup) and 18."""
    for family in FAMILIES:
        for n, G, H in ((1, 1, 1), (1, 1, 3), (1, 2, 2), (1, 5, 1), (2, 3, 3)):
            _run_attention(gpu, n=n, G=G, H=H, D=64, T=T, layout='time' if G > 1 else 'contig', cls=cls, family=family, seed=T, pad=(8, 8) if H == 3 else (0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['marked', 'sharp', 'negative'])
def test_tiny_time_layout_product_geometry(gpu, family):
    """Motionformer time attention: 196 groups of 8 tokens, token stride 196, + CLS key."""
    _run_attention(gpu, n=2, G=196, H=3, D=64, T=8, layout='time', cls='first', family=family, seed=4)


# ======================================================================================================================================
# 3. sf_attention_cls_partial (attn_tiny64_kernel<true>, attn_mfma_kernel with the CLS query in the free query slot)
# ======================================================================================================================================
def _run_partial(gpu, keep=None, **kw):
    """sf_attention_cls_partial[_masked]: records per (sequence, head, group), token rows within their bars and bit-identical to sf_attention[_masked] on the same inputs,
    the CLS row untouched; then sf_attention_cls_combine[_stats] against the reference's CLS row and (M, L)."""
    run = _Run(gpu, **kw)
    name = _kernel_name(run) + ' + CLS query'
    ref = run.ref(keep, cls_query=True)
    out, part = run.partial(keep)
    run.check_tokens(name, out, ref)                                               # ... which also asserts that the CLS row kept its canary
    plain = run.attention(keep)
    assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), f'{name}: token rows differ from sf_attention'
    rec = part.cpu().double().view(run.n, run.H, run.G, 66)
    _check_records(name, rec, ref['rec'])
    stats = torch.full((run.n * run.H * 2,), float('nan'), device=gpu)
    _ok(_lib().sf_attention_cls_combine_stats(part.data_ptr(), run.G, out.data_ptr(), run.ldo, run.R, run.cls_row, run.n, run.H, stats.data_ptr(), _st()), 'combine_stats')
    out2 = plain.clone()
    _ops().attention_cls_combine(part, out2, n_part=run.G, n_seq=run.n, out_seq_rows=run.R, out_row=run.cls_row, heads=run.H)
    torch.cuda.synchronize()
    assert not ref['row_dead'].any()
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), 'sf_attention_cls_combine and _combine_stats differ'
    _check_section('partial + combine', 'CLS row', run.cls_row_of(out), ref['row'])
    _check_stats('partial + combine', stats.cpu().double().view(run.n, run.H, 2), ref)
    run.check_tokens(name, out, ref, cls_written=True)
    return run, ref, rec


@pytest.mark.gpu
@pytest.mark.parametrize('T', list(range(1, 9)) + [9, 15, 17, 24, 31, 97, 104, 111, 193, 196, 200, 207])
def test_cls_partial(gpu, T):
    """Tiny path (n_tok 1 .. 8, fp32: A_rec = 0) and MFMA path (n_tok % 16 in {1, 8, 15} at NKT 2, 7, 13, and 9, 15, 196, 200; bf16-packed exponentials: A_rec =
    sum_k e_k |v_kd| for o, none for l, which is summed before the packing).  Three groups: the CLS key (marked in a column of its own) counts in group 0 only."""
    for i, family in enumerate(FAMILIES):
        _run_partial(gpu, n=2, G=3, H=3, D=64, T=T, layout='time' if (T + i) % 2 else 'contig', cls='first', family=family, seed=T + i, pad=(8, 8) if i % 2 else (0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [dict(n=2, G=196, H=3, T=8, layout='time'), dict(n=2, G=8, H=12, T=196, layout='contig'), dict(n=1, G=49, H=2, T=8, layout='time')],
                         ids=['time', 'space', 'time-block'])
def test_cls_partial_combine_product_geometries(gpu, kw):
    """partial + combine end to end at the time (196 records: the serial combine path) and space (8 records) geometries of the model, and 49 records."""
    for family in ('marked', 'sharp'):
        _run_partial(gpu, D=64, cls='first', family=family, seed=6, **kw)


@pytest.mark.gpu
def test_cls_partial_rejections(gpu):
    run = _Run(gpu, n=1, G=2, H=1, D=64, T=16)
    q, k, v = run.views()
    out = run.canary.clone().to(gpu)
    part = torch.zeros(4 * 66, device=gpu)
    fn = _lib().sf_attention_cls_partial

    def call(T=16, cls_row=0, D=64, p=part):
        return fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), run.ld, out.data_ptr(), run.ldo, 1, run.R, 2, 1, T, 1, T, cls_row, 1, D, 0.125, p.data_ptr() if p is not None else None, _st())

    _rejected(call(), 'n_tok % 16 == 0')
    _rejected(call(T=15, cls_row=-1), 'cls_row < 0')
    _rejected(call(T=15, D=96), 'head_dim 96')
    _rejected(call(T=15, p=None), 'no partial buffer')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int16), run.canary.view(torch.int16))


# ======================================================================================================================================
# 4. sf_attention_cls_combine / _combine_stats / _combine_mx on synthetic records
# ======================================================================================================================================
def _records(n, H, P, seed, peak='random', empty=()):
    """(n, H, P, 66) fp32 records: maxima spread over +-100 (most weights underflow to 0), l in [1, 9), o = l * N(0, 1); `empty` records are (-inf, 0, 0)."""
    g = _gen(seed)
    m = (torch.rand(n, H, P, generator=g) * 200 - 100)
    near = torch.rand(n, H, P, generator=g) < 0.3                                  # a third of them within 8 of the top: several weights that matter
    m = torch.where(near, 92 + 8 * torch.rand(n, H, P, generator=g), m)
    if peak == 'first':
        m[..., 0] = 101.0
    elif peak == 'last':
        m[..., -1] = 101.0
    l = 1 + 8 * torch.rand(n, H, P, generator=g)
    o = torch.randn(n, H, P, 64, generator=g) * l[..., None]
    rec = torch.cat([m[..., None], l[..., None], o], -1).float()
    for i in empty:
        rec[:, :, i, 0], rec[:, :, i, 1:] = -math.inf, 0.0
    return rec


def _combine_ref(rec):
    """float64 merge of (n, H, P, 66) records: row, (M, L), element bar and fp32 term (module docstring)."""
    r = rec.double()
    m, l, o = r[..., 0], r[..., 1], r[..., 2:]
    P = m.shape[-1]
    M = m.amax(-1)
    gap = torch.where(m == -math.inf, torch.zeros_like(m), (m - M[..., None]).abs())
    w = torch.exp2(m - M[..., None])
    L = (l * w).sum(-1)
    ref = (o * w[..., None]).sum(2) / L[..., None]
    we = w * (gap + 2) * U32                                                       # the weights' fp32 error: the argument's rounding, v_exp_f32
    F = ((P + 8) * U32 * (o.abs() * w[..., None]).sum(2) + (o.abs() * we[..., None]).sum(2)) / L[..., None] + ref.abs() * ((P + 8) * U32 + (l * we).sum(-1, keepdim=True) / L[..., None])
    Lbar = MARGIN * ((P + 8) * U32 * L + (l * we).sum(-1))
    return _Sec(ref, MARGIN * (U * ref.abs() + F), _rb(ref), F), M, L, Lbar


def _combine(gpu, rec, out_rows=3, out_row=1, pad=8):
    n, H, P = rec.shape[:3]
    ldo = H * 64 + pad
    can = _canary(n * out_rows, ldo, P)
    out = can.clone().to(gpu)
    stats = torch.full((n * H * 2,), float('nan'), device=gpu)
    part = rec.contiguous().view(-1).to(gpu)
    _ok(_lib().sf_attention_cls_combine_stats(part.data_ptr(), P, out.data_ptr(), ldo, out_rows, out_row, n, H, stats.data_ptr(), _st()), 'sf_attention_cls_combine_stats')
    out2 = can.clone().to(gpu)
    _ops().attention_cls_combine(part, out2, n_part=P, n_seq=n, out_seq_rows=out_rows, out_row=out_row, heads=H)
    torch.cuda.synchronize()
    raw = out.cpu()
    assert torch.equal(raw.view(torch.int16), out2.cpu().view(torch.int16)), 'sf_attention_cls_combine and _combine_stats differ'
    written = torch.zeros(n, out_rows, ldo, dtype=torch.bool)
    written[:, out_row, :H * 64] = True
    _assert_untouched(raw, can, written.view(n * out_rows, ldo), 'attn_cls_combine64_kernel')
    got = raw.double().view(n, out_rows, ldo)[:, out_row, :H * 64].reshape(n, H, 64)
    return got, stats.cpu().double().view(n, H, 2), part


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 2, 8, 33, 49, 63, 64, 65, 196, 1000])
@pytest.mark.parametrize('peak,empty', [('random', ()), ('first', (1,)), ('last', (0, 2, 3))], ids=['random', 'peak-first-one-empty', 'peak-last-three-empty'])
def test_cls_combine_synthetic(gpu, P, peak, empty):
    """attn_cls_combine64_kernel on records that no attention kernel made, against float64: wave-reduction path (n_part <= 64) and serial path (> 64); maxima spread over
    +-100, empty records (-inf, 0, 0), the maximum in the first / last record; out_row 1 of 3, padded ldo.  M is a maximum of fp32 numbers: exact."""
    empty = tuple(i for i in empty if i < P - 1) if peak == 'last' else tuple(i for i in empty if 0 < i < P)
    rec = _records(2, 3, P, P, peak, empty)
    sec, M, L, Lbar = _combine_ref(rec)
    got, st, _ = _combine(gpu, rec)
    kernel = 'attn_cls_combine64_kernel ' + ('(n_part <= 64)' if P <= 64 else '(n_part > 64)')
    _check_section(kernel, 'merged row', got, sec)
    assert torch.equal(st[..., 0], M), f'{kernel}: M is not the maximum of the records'
    rl = ((st[..., 1] - L).abs() / Lbar).max().item()
    _worst(kernel + ' L', rl)
    assert rl <= 1.0, f'{kernel}: L outside its bar (ratio {rl:.3g})'


@pytest.mark.gpu
def test_cls_combine_paths_agree(gpu):
    """The same 64 records through the wave-reduction path and, padded with an empty 65th record, through the serial path: both within the bar of the one float64 merge
    (two bf16 roundings of nearly equal fp32 numbers may fall on either side of a tie, so the outputs need not be bit-equal), M bit-equal."""
    rec = _records(2, 3, 64, 77)
    rec65 = torch.cat([rec, _records(2, 3, 1, 0, empty=(0,))], 2)
    sec, M, L, Lbar = _combine_ref(rec)
    a, sa, _ = _combine(gpu, rec)
    b, sb, _ = _combine(gpu, rec65)
    _check_section('attn_cls_combine64_kernel (n_part <= 64)', 'merged row', a, sec)
    _check_section('attn_cls_combine64_kernel (n_part > 64)', 'merged row', b, sec)
    assert ((a - b).abs() <= 2 * sec.bar).all()
    assert torch.equal(sa[..., 0], sb[..., 0]) and ((sa[..., 1] - sb[..., 1]).abs() <= 2 * Lbar).all()


@pytest.mark.gpu
@pytest.mark.parametrize('P', [8, 49, 64, 65, 196])
def test_cls_combine_mx_equals_quantized_combine(gpu, P):
    """sf_attention_cls_combine_mx byte-equal (e4m3 bytes and scale planes; rows it does not own keep their fill) to sf_quantize_mxfp8 of sf_attention_cls_combine on
    the same records; 4 heads (even), one sequence whose records are all zero in o: an all-zero row, the zero-amax scale byte."""
    ops = _ops()
    n, H, rows, out_row = 3, 4, 5, 2
    rec = _records(n, H, P, 200 + P, empty=(1,) if P > 2 else ())
    rec[1, :, :, 2:] = 0.0
    part = rec.contiguous().view(-1).to(gpu)
    out = torch.zeros(n * rows, H * 64, device=gpu, dtype=BF)
    ops.attention_cls_combine(part, out, n_part=P, n_seq=n, out_seq_rows=rows, out_row=out_row, heads=H)
    q0, s0 = torch.full((n * rows, H * 64), 7, device=gpu, dtype=torch.uint8), ops.mx_scale_planes(n * rows, H * 64, gpu)
    ops.quantize_mxfp8(out, q0, s0)
    q1, s1 = torch.full((n * rows, H * 64), 7, device=gpu, dtype=torch.uint8), ops.mx_scale_planes(n * rows, H * 64, gpu)
    s1.fill_(9)
    ops.attention_cls_combine_mx(part, q1, s1, n_part=P, n_seq=n, out_seq_rows=rows, out_row=out_row, heads=H)
    torch.cuda.synchronize()
    own = torch.zeros(n * rows, dtype=torch.bool, device=gpu)
    own[torch.arange(n, device=gpu) * rows + out_row] = True
    assert torch.equal(q1[own], q0[own]) and (q1[~own] == 7).all()
    assert torch.equal(s1[:, :n * rows][:, own], s0[:, :n * rows][:, own]) and (s1[:, :n * rows][:, ~own] == 9).all() and (s1[:, n * rows:] == 9).all()
    assert (out.view(n, rows, -1)[1, out_row] == 0).all()


# ======================================================================================================================================
# 5. sf_attention_cls / sf_attention_cls_stats / sf_attention_cls_masked (attn_cls64_kernel)
# ======================================================================================================================================
def _run_cls(gpu, n_keys, family='flat', kv_row0=0, extra=0, q_row=0, out_row=0, out_rows=1, H=3, n=2, peak=None, keep=None, seed=0, compare_unmasked=False):
    """One launch of sf_attention_cls_stats (or sf_attention_cls_masked) with q in a buffer of its own (sequence stride q_rows), k | v in a packed buffer (sequence stride
    kv_rows > n_keys), the output with a third stride; against float64 over the keys kv_row0 .. kv_row0 + n_keys - 1 (minus the masked ones)."""
    D, Hd = 64, H * 64
    kv_rows, q_rows = kv_row0 + n_keys + extra, q_row + 2
    geo = (1, kv_row0, 0, 1, n_keys, -1)
    kvh = _inputs(n, kv_rows, geo, H, D, family, 300 + seed, 3 * Hd + 8)
    g = _gen(400 + seed)
    sig = {'flat': 0.25, 'marked': 0.25, 'sharp': 10.0, 'negative': 1.0, 'plain': 1.0}[family]
    qh = torch.randn(n * q_rows, 3 * Hd + 8, generator=g) * sig                   # a buffer of its own (other sequence stride), the row stride the ABI shares with k | v
    kv3 = kvh.view(n, kv_rows, -1)
    if family == 'negative':                                                       # every score about -5
        qh.view(n, q_rows, -1)[:, q_row, :Hd] -= kv3[:, kv_row0:kv_row0 + n_keys, Hd:2 * Hd].float().mean(1)
    if peak is not None:                                                           # the query is 6 x one key: that key dominates
        j = kv_row0 + (n_keys - 1 if peak == 'last' else 0)
        qh.view(n, q_rows, -1)[:, q_row, :Hd] = 6 * kv3[:, j, Hd:2 * Hd].float()
    qh = qh.to(BF)
    qd, kvd = qh.to(gpu), kvh.to(gpu)
    ldo = Hd + 16
    can = _canary(n * out_rows, ldo, seed)
    out = can.clone().to(gpu)
    stats = torch.full((n * H * 2,), float('nan'), device=gpu)
    k, v = kvd[:, Hd:2 * Hd], kvd[:, 2 * Hd:3 * Hd]
    args = (qd.data_ptr(), q_rows, q_row, k.data_ptr(), v.data_ptr(), kvd.stride(0), kv_rows, kv_row0, n_keys, out.data_ptr(), ldo, out_rows, out_row, n, H, 64, 0.125)
    if keep is None:
        _ok(_lib().sf_attention_cls_stats(*args, stats.data_ptr(), _st()), 'sf_attention_cls_stats')
        out2 = can.clone().to(gpu)
        _ops().attention_cls(qd[:, :Hd], k, v, out2, n_seq=n, q_seq_rows=q_rows, q_row=q_row, kv_seq_rows=kv_rows, kv_row0=kv_row0, n_keys=n_keys, out_seq_rows=out_rows,
                             out_row=out_row, heads=H, head_dim=64, scale=0.125)
    else:
        out2 = None
        _ops().attention_cls(qd[:, :Hd], k, v, out, n_seq=n, q_seq_rows=q_rows, q_row=q_row, kv_seq_rows=kv_rows, kv_row0=kv_row0, n_keys=n_keys, out_seq_rows=out_rows,
                             out_row=out_row, heads=H, head_dim=64, scale=0.125, key_keep=keep.to(torch.uint8).contiguous().view(-1).to(gpu))
    torch.cuda.synchronize()
    raw = out.cpu()
    if out2 is not None:
        assert torch.equal(raw.view(torch.int16), out2.cpu().view(torch.int16)), 'sf_attention_cls and sf_attention_cls_stats differ'
    x = kvh.double().view(n, kv_rows, -1)
    K = x[:, kv_row0:kv_row0 + n_keys, Hd:2 * Hd].reshape(n, n_keys, H, 64).transpose(1, 2)
    V = x[:, kv_row0:kv_row0 + n_keys, 2 * Hd:3 * Hd].reshape(n, n_keys, H, 64).transpose(1, 2)
    Q = qh.double().view(n, q_rows, -1)[:, q_row, :Hd].reshape(n, H, 1, 64)
    mask = torch.ones(n, n_keys, dtype=torch.bool) if keep is None else keep.view(n, kv_rows)[:, kv_row0:kv_row0 + n_keys].bool()
    depth = (n_keys + 31) // 32 + 8
    r = _attend(Q, K, V, mask[:, None, None, :], 0.125, packs_p=False, depth=depth, chain=True)
    assert not r['dead'].any()
    r1 = {key: (val[:, :, 0] if val.dim() >= 3 else val) for key, val in r.items()}
    sec = _direct(r1['o'], r1['A'], r1['F'], r1['emu'])
    got = raw.double().view(n, out_rows, ldo)[:, out_row, :Hd].reshape(n, H, 64)
    assert torch.isfinite(got).all()
    kernel = 'attn_cls64_kernel' + (' (masked)' if keep is not None else '')
    res = _check_section(kernel, 'CLS row', got, sec)
    written = torch.zeros(n, out_rows, ldo, dtype=torch.bool)
    written[:, out_row, :Hd] = True
    _assert_untouched(raw, can, written.view(n * out_rows, ldo), kernel)
    if keep is None:
        M, L, Mbar, Lbar = _stats_bars(r1, 64, n_keys, depth=depth + 8)
        _check_stats(kernel, stats.cpu().double().view(n, H, 2), dict(M=M, L=L, Mbar=Mbar, Lbar=Lbar))
    return res, raw, can


CLS_KEYS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 1569]


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys', CLS_KEYS)
@pytest.mark.parametrize('family', FAMILIES)
def test_cls_query(gpu, n_keys, family):
    """attn_cls64_kernel is fp32 up to its store (A = 0); 32 keys per step over 4 waves x 8 slots, so n_keys < 32 leaves empty slots (m = -inf) in the merges and 1569
    walks 50 steps.  Once with everything at row 0 and once with kv_row0 = 3 inside longer sequences, q_row 1, out_row 2 of 4; statistics (M, L) against float64."""
    _run_cls(gpu, n_keys, family, seed=n_keys)
    _run_cls(gpu, n_keys, family, kv_row0=3, extra=2, q_row=1, out_row=2, out_rows=4, seed=n_keys + 1)


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys', [9, 33, 65, 255, 1569])
@pytest.mark.parametrize('peak', ['first', 'last'])
def test_cls_query_dominant_key(gpu, n_keys, peak):
    """The query is 6 x the last key (every earlier partial state of that slot, and every other slot, is rescaled to ~0) or 6 x key 0."""
    _run_cls(gpu, n_keys, 'marked', peak=peak, kv_row0=2, extra=1, seed=n_keys)


# ======================================================================================================================================
# 6. masks: sf_attention_masked, sf_attention_cls_partial_masked, sf_attention_cls_masked
# ======================================================================================================================================
def _mask(run, pattern, ref=None):
    """keep (n, R) bool for one of the patterns of the issue; every pattern but 'dead*' leaves each group a kept key."""
    n, R, G, T, cls_row = run.n, run.R, run.G, run.T, run.cls_row
    has_cls = 1 if cls_row >= 0 else 0
    nk = T + has_cls
    keep = torch.ones(n, R, dtype=torch.bool)
    slot_row = lambda g, j: cls_row if (has_cls and j == 0) else int(run.idx[g, j - has_cls])   # noqa: E731
    if pattern in ('rand20', 'rand80'):
        keep = torch.rand(n, R, generator=_gen(T)) >= (0.2 if pattern == 'rand20' else 0.8)
        if has_cls:
            keep[:, cls_row] = True
        else:
            keep[:, run.idx[:, 0]] = True
    elif pattern == 'last_key':
        keep[:, run.idx[:, -1]] = False
    elif pattern == 'tile_key0':                                                    # key 0 of the last tile (of tile 0 without a CLS key when there is one tile)
        j = 16 * ((nk - 1) // 16)
        for g in range(G):
            keep[:, slot_row(g, j) if (j or not has_cls) else int(run.idx[g, 0])] = False
    elif pattern == 'group':                                                        # every token of group 1 (sequence 0 only): its queries see the CLS key alone
        keep[0, run.idx[1]] = False
    elif pattern == 'cls':
        keep[:, cls_row] = False
    elif pattern == 'tile':                                                         # a whole key tile (the second, or what there is of tile 0 beyond key 0)
        lo, hi = (16, 32) if nk > 32 else (1, min(nk - 1, 16))
        for g in range(G):
            for j in range(lo, hi):
                keep[:, slot_row(g, j)] = False
    elif pattern == 'dominant':                                                     # the key that dominates query 0 of head 0 in every group
        q, k, _ = run.wide()
        for s in range(n):
            for g in range(G):
                rows = [slot_row(g, j) for j in range(nk)]
                sc = (k[s, rows, 0] * q[s, int(run.idx[g, 0]), 0][None]).sum(-1)
                keep[s, rows[int(sc.argmax())]] = False
    elif pattern == 'dead_nocls':                                                   # no CLS key: group 1 of sequence 0 keeps nothing
        keep[0, run.idx[1]] = False
    elif pattern == 'dead_cls':                                                     # group 1 of sequence 0 and the CLS key of sequence 0
        keep[0, run.idx[1]] = False
        keep[0, cls_row] = False
    else:
        assert pattern == 'ones'
    return keep


MASK_SHAPES = [(64, 8), (64, 14), (64, 31), (64, 105), (64, 200), (96, 185), (96, 207)]     # tiny; MFMA D = 64 at NKT 1, 2, 7, 13; D = 96 at NKT 12, 13 (with the CLS key); nk % 16 = 0 and != 0


@pytest.mark.gpu
@pytest.mark.parametrize('D,T', MASK_SHAPES)
@pytest.mark.parametrize('pattern', ['rand20', 'rand80', 'last_key', 'tile_key0', 'group', 'cls', 'tile', 'dominant'])
def test_attention_masked(gpu, D, T, pattern):
    """sf_attention_masked against float64 with -inf masks on both paths.  'group': the queries of a fully masked group see the CLS key alone, p = 1 exactly and the
    output is v_cls bit for bit (exp2(0) = 1, l = 1, bf16(1) = 1, one product with a bf16 number)."""
    for i, family in enumerate(('sharp',) if pattern == 'dominant' else ('marked', 'negative', 'sharp')):
        run = _Run(gpu, n=2, G=3, H=3, D=D, T=T, layout='time' if i % 2 else 'contig', cls='first', family=family, seed=T + i, pad=(8, 8))
        keep = _mask(run, pattern, run.ref() if pattern == 'dominant' else None)
        ref = run.ref(keep)
        out = run.attention(keep)
        run.check_tokens(_kernel_name(run) + ' (masked)', out, ref)
        if pattern == 'group':
            Hd = run.Hd
            vcls = run.qkv_h.view(run.n, run.R, run.ld)[0, 0, 2 * Hd:3 * Hd]
            rows = out.cpu().view(run.n, run.R, run.ldo)[0, run.idx[1], :Hd]
            assert torch.equal(rows.view(torch.int16), vcls.view(torch.int16)[None].expand_as(rows)), 'a query that sees the CLS key alone must return v_cls exactly'


@pytest.mark.gpu
@pytest.mark.parametrize('D,T', MASK_SHAPES)
def test_attention_masked_no_cls_and_all_ones(gpu, D, T):
    """Without a CLS key (random masks, every group keeps its first token), and the all-ones mask: bit-identical to the unmasked entry point."""
    for cls in ('none', 'first'):
        run = _Run(gpu, n=2, G=3, H=3, D=D, T=T + (1 if cls == 'none' and T in (31, 207) else 0), layout='time', cls=cls, family='marked', seed=T)
        if cls == 'none':
            for pattern in ('rand20', 'rand80'):
                keep = _mask(run, pattern)
                run.check_tokens(_kernel_name(run) + ' (masked)', run.attention(keep), run.ref(keep))
        ones = run.attention(_mask(run, 'ones'))
        assert torch.equal(ones.view(torch.int16), run.attention().view(torch.int16)), 'an all-ones mask must not change a bit'


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['dead_nocls', 'dead_cls'])
def test_masked_dead_group(gpu, case):
    """The two cases in which rows are left out of the comparison: one group of one sequence keeps no key at all (0 / 0 in the reference as well).  Exactly those rows
    are excluded, they are the only rows that may be non-finite, every other element of the output is compared."""
    T = 31 if case == 'dead_nocls' else 8                                          # attn_mfma_kernel without a CLS key, attn_tiny64_kernel with a masked CLS key
    run = _Run(gpu, n=2, G=3, H=3, D=64, T=T, layout='contig', cls='none' if case == 'dead_nocls' else 'first', family='marked', seed=T)
    keep = _mask(run, case)
    ref = run.ref(keep)
    assert int(ref['dead'].sum()) == 1 and bool(ref['dead'][0, 1])
    run.check_tokens(_kernel_name(run) + ' (masked)', run.attention(keep), ref, case=case)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [14, 31, 105, 200])
@pytest.mark.parametrize('pattern', ['rand20', 'rand80', 'last_key', 'tile_key0', 'group', 'cls', 'tile', 'dominant', 'ones'])
def test_cls_partial_masked(gpu, T, pattern):
    """sf_attention_cls_partial_masked (MFMA path only): records, token rows, merged row and (M, L) against float64 with -inf masks.  'group': the record of the group
    without a kept key is merge-neutral (l = 0, o = 0, nothing NaN) and the merged row is the reference over the remaining groups.  'ones': records and outputs
    bit-identical to sf_attention_cls_partial."""
    family = 'sharp' if pattern == 'dominant' else ('marked' if T % 2 else 'negative')
    kw = dict(n=2, G=3, H=3, D=64, T=T, layout='time' if T > 100 else 'contig', cls='first', family=family, seed=T, pad=(8, 8))
    probe = _Run(gpu, **kw)
    keep = _mask(probe, pattern, probe.ref() if pattern == 'dominant' else None)
    run, ref, rec = _run_partial(gpu, keep=keep, **kw)
    if pattern == 'group':
        assert bool(ref['rec']['empty'][0, :, 1].all()) and int(ref['rec']['empty'].sum()) == run.H
    if pattern == 'ones':
        out0, part0 = run.partial()
        out1, part1 = run.partial(keep)
        assert torch.equal(out0.view(torch.int16), out1.view(torch.int16)) and torch.equal(part0.view(torch.int32), part1.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys', [9, 33, 64, 255, 1569])
def test_cls_query_masked(gpu, n_keys):
    """sf_attention_cls_masked against float64: random 20 % / 80 %, the first 32-key step masked whole, the dominant key masked; all-ones bit-identical to sf_attention_cls."""
    kv_row0, extra = 2, 1
    kv_rows = kv_row0 + n_keys + extra
    g = _gen(n_keys)
    for frac in (0.2, 0.8):
        keep = torch.rand(2, kv_rows, generator=g) >= frac
        keep[:, kv_row0 + n_keys // 2] = True
        _run_cls(gpu, n_keys, 'marked', kv_row0=kv_row0, extra=extra, keep=keep, seed=n_keys)
    keep = torch.ones(2, kv_rows, dtype=torch.bool)
    keep[:, kv_row0:kv_row0 + min(32, n_keys - 1)] = False
    _run_cls(gpu, n_keys, 'negative', kv_row0=kv_row0, extra=extra, keep=keep, seed=n_keys)
    keep = torch.ones(2, kv_rows, dtype=torch.bool)
    keep[:, kv_row0 + n_keys - 1] = False                                          # peak='last': the dominant key
    _run_cls(gpu, n_keys, 'marked', kv_row0=kv_row0, extra=extra, keep=keep, peak='last', seed=n_keys)
    _, a, _ = _run_cls(gpu, n_keys, 'marked', kv_row0=kv_row0, extra=extra, keep=torch.ones(2, kv_rows, dtype=torch.bool), seed=n_keys)
    _, b, _ = _run_cls(gpu, n_keys, 'marked', kv_row0=kv_row0, extra=extra, seed=n_keys)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), 'an all-ones mask must not change a bit'


# ======================================================================================================================================
# 7. sf_attention_cls_partial_mx
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('T', [193, 196, 200, 207])
@pytest.mark.parametrize('H', [2, 12])
def test_cls_partial_mx(gpu, T, H):
    """attn_mfma_kernel<64, 13, true>: e4m3 bytes and scale planes byte-equal to sf_quantize_mxfp8 of sf_attention_cls_partial's bf16 output (itself compared with float64
    in section 3), records bit-equal, rows it does not own (the CLS row, rows behind the sequences) keep their fill.  A few rows scaled by 40, one all-zero 32-column
    value block."""
    ops = _ops()
    n, G = 2, 3
    run = _Run(gpu, n=n, G=G, H=H, D=64, T=T, layout='contig', cls='first', family='plain', seed=T + H, pad=(8, 0), extra=0)
    Hd, rows = run.Hd, n * run.R
    run.qkv[5:9] *= 40.0
    run.qkv[:, 2 * Hd + 64:2 * Hd + 96] = 0
    q, k, v = run.views()
    kw = run.kw()
    out = torch.zeros(rows, Hd, device=gpu, dtype=BF)
    part = torch.full((n * H * G * 66,), float('nan'), device=gpu)
    ops.attention_cls_partial(q, k, v, out, part, **kw)
    q0, s0 = torch.empty(rows, Hd, device=gpu, dtype=torch.uint8), ops.mx_scale_planes(rows, Hd, gpu)
    ops.quantize_mxfp8(out, q0, s0)
    q1, s1 = torch.full((rows + 3, Hd), 7, device=gpu, dtype=torch.uint8), ops.mx_scale_planes(rows, Hd, gpu)
    s1.fill_(9)
    part1 = torch.full_like(part, float('nan'))
    kw.pop('head_dim')
    ops.attention_cls_partial_mx(q, k, v, q1, s1, part1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(part.view(torch.int32), part1.view(torch.int32)), 'records differ from sf_attention_cls_partial'
    own = torch.zeros(n, run.R, dtype=torch.bool)
    own[:, run.idx.flatten()] = True
    own = own.view(-1).to(gpu)
    assert torch.equal(q1[:rows][own], q0[own]) and (q1[:rows][~own] == 7).all() and (q1[rows:] == 7).all()
    assert torch.equal(s1[:, :rows][:, own], s0[:, :rows][:, own]) and (s1[:, :rows][:, ~own] == 9).all() and (s1[:, rows:] == 9).all()


@pytest.mark.gpu
def test_cls_partial_mx_rejections(gpu):
    """13 key tiles with a free query slot: n_tok 193 .. 207.  192 (n_tok % 16 == 0) and 208 (14 tiles) are refused, as are an odd head count and cls_row < 0."""
    run = _Run(gpu, n=1, G=1, H=2, D=64, T=207, layout='contig', cls='first')
    q, k, v = run.views()
    rows = run.R
    q1, s1 = torch.full((rows, 128), 7, device=gpu, dtype=torch.uint8), _ops().mx_scale_planes(rows, 128, gpu)
    part = torch.zeros(2 * 66, device=gpu)
    fn = _lib().sf_attention_cls_partial_mx

    def call(T, cls_row=0, H=2):
        return fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), run.ld, q1.data_ptr(), 128, s1.data_ptr(), s1.stride(0), 1, rows, 1, 1, T, 1, T, cls_row, H, 0.125, part.data_ptr(), _st())

    for T in (192, 208, 191, 176):
        _rejected(call(T), f'n_tok {T}')
    _rejected(call(207, cls_row=-1), 'cls_row < 0')
    _rejected(call(207, H=1), 'odd head count')
    torch.cuda.synchronize()
    assert (q1 == 7).all() and (s1 == 0).all()


# ======================================================================================================================================
# 8. argument edges
# ======================================================================================================================================
@pytest.mark.gpu
def test_attention_argument_edges(gpu):
    """n_seq = 0 returns 0 and writes nothing; nk = 209, head_dim 32, a misaligned pointer, ld % 8 != 0 and seq_rows * ld >= 2^31 are refused with a message."""
    run = _Run(gpu, n=1, G=1, H=1, D=64, T=20, layout='contig', cls='first', pad=(8, 8))
    q, k, v = run.views()
    out = run.canary.clone().to(gpu)
    fn = _lib().sf_attention

    def call(qp=None, ld=None, ldo=None, n_seq=1, seq_rows=None, T=20, cls_row=0, D=64, outp=None):
        return fn(qp or q.data_ptr(), k.data_ptr(), v.data_ptr(), ld or run.ld, outp or out.data_ptr(), ldo or run.ldo, n_seq, seq_rows or run.R, 1, 1, T, 1, T, cls_row, 1, D,
                  0.125, _st())

    assert call(n_seq=0) == 0
    _rejected(call(T=208), 'nk = 209')
    _rejected(call(T=209, cls_row=-1), 'n_tok = 209')
    _rejected(call(T=0), 'n_tok = 0')
    _rejected(call(D=32), 'head_dim 32')
    _rejected(call(qp=q.data_ptr() + 2), 'misaligned q')
    _rejected(call(outp=out.data_ptr() + 8), 'misaligned out')
    _rejected(call(ld=run.ld + 4), 'ld % 8 != 0')
    _rejected(call(ldo=run.ldo + 2), 'ldo % 8 != 0')
    _rejected(call(seq_rows=(2 ** 31) // run.ld + 1), 'seq_rows * ld >= 2^31')
    _rejected(call(seq_rows=2 ** 24), 'seq_rows >= 2^24')
    fc = _lib().sf_attention_cls
    assert fc(q.data_ptr(), run.R, 0, k.data_ptr(), v.data_ptr(), run.ld, run.R, 0, 5, out.data_ptr(), run.ldo, run.R, 0, 0, 1, 64, 0.125, _st()) == 0
    _rejected(fc(q.data_ptr(), run.R, 0, k.data_ptr(), v.data_ptr(), run.ld, run.R, 0, 5, out.data_ptr(), run.ldo, run.R, 0, 1, 1, 96, 0.125, _st()), 'cls head_dim 96')
    _rejected(fc(q.data_ptr(), run.R, 0, k.data_ptr(), v.data_ptr(), run.ld, run.R, 0, 0, out.data_ptr(), run.ldo, run.R, 0, 1, 1, 64, 0.125, _st()), 'cls n_keys 0')
    part = torch.zeros(66, device=gpu)
    assert _lib().sf_attention_cls_combine(part.data_ptr(), 1, out.data_ptr(), run.ldo, 1, 0, 0, 1, _st()) == 0
    _rejected(_lib().sf_attention_cls_combine(part.data_ptr(), 0, out.data_ptr(), run.ldo, 1, 0, 1, 1, _st()), 'combine n_part 0')
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int16), run.canary.view(torch.int16))


@pytest.mark.gpu
def test_attention_offsets_above_2_30(gpu):
    """One sequence of 1,398,100 rows x ld 1536 (seq_rows * ld = 2^31 - 2048, the largest the launcher accepts; about 4 GiB, zero but for the touched rows) whose two
    groups are its last rows: their element offsets exceed 2^30 in q | k | v and in the output (ldo 1024) - the 24-bit multiply / 32-bit offset addressing of
    attn_mfma_kernel.  The CLS key is row 0.  Compared with float64 on those rows; every other output element keeps its canary."""
    seq_rows, ld, ldo, H, D, G, T = 1398100, 1536, 1024, 2, 64, 2, 40
    Hd = H * D
    assert seq_rows * ld < 2 ** 31 and (seq_rows - G * T - 3) * ldo > 2 ** 30
    small_geo, small_R = _geometry(G, T, 'contig', 'first', extra=0)
    small = _inputs(1, small_R, small_geo, H, D, 'marked', 9, 3 * Hd)
    row0 = seq_rows - G * T - 3
    geo = (G, row0, T, 1, T, 0)
    rows = torch.cat([torch.zeros(1, dtype=torch.int64), row0 + torch.arange(G * T)])
    big = torch.zeros(seq_rows, ld, device=gpu, dtype=BF)
    big[rows.to(gpu), :3 * Hd] = small.to(gpu)
    can = (0x4000 + (torch.arange(seq_rows, device=gpu, dtype=torch.int32)[:, None] * 5 + torch.arange(ldo, device=gpu, dtype=torch.int32)[None] * 37) % 128).to(torch.int16)
    out = can.clone().view(BF)
    try:
        _ops().attention(big[:, :Hd], big[:, Hd:2 * Hd], big[:, 2 * Hd:3 * Hd], out, n_seq=1, seq_rows=seq_rows, n_groups=G, row0=row0, group_stride=T, tok_stride=1, n_tok=T,
                         cls_row=0, heads=H, head_dim=D, scale=0.125)
        torch.cuda.synchronize()
        tok_rows = rows[1:].to(gpu)
        got = out[tok_rows, :Hd].cpu().double().view(1, G, T, H, D).permute(0, 1, 3, 2, 4)
        outi = out.view(torch.int16)
        outi[tok_rows, :Hd] = can[tok_rows, :Hd]
        assert torch.equal(outi, can), 'an element outside the token rows changed'
    finally:
        del big, can, out
        torch.cuda.empty_cache()
    x = small.double().view(1, small_R, 3, H, D)
    ref = grouped_attention_fwd_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], small_geo, 0.125)
    assert geo[0] == small_geo[0] and torch.isfinite(got).all()
    _check_section('attn_mfma_kernel<64>', 'token rows above 2^30', got, ref['tok'], key_shift=1)


@pytest.mark.gpu
def test_zz_report_worst_ratios(gpu):
    """Prints the worst observed error / bar ratio per kernel of this run (pytest -s); asserts that rows were left out of a comparison in at most two cases."""
    for name in sorted(WORST):
        print(f'worst ratio  {name}: {WORST[name]:.3f}')
    assert len(EXCLUDED) <= 2, sorted(EXCLUDED)
