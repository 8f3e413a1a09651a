"""Float64 oracle of the grouped attention backward (sf_attention_group_bwd / sf_attention_tiny_bwd, their _clsq forms, sf_attention_cls_bwd): the exact result,
the element bars, the bf16 emulation and the fp32 terms, shared by tests/test_attention_bwd_gpu.py (kernel by kernel) and tests/tower_bwd_oracle.py (inside the
stepped tower backward).  Pure torch; every tensor is made on the device of q.  The bars are derived in the docstring of test_attention_bwd_gpu.py."""
import torch

U = 2.0 ** -8             # bf16 unit roundoff of the bars
U32 = 2.0 ** -24          # fp32 unit roundoff
MARGIN = 1.5              # second-order terms and v_exp_f32, once on the whole bar
LOG2E = 1.4426950408889634
BF = torch.bfloat16


def _rb(x):
    """float64 -> nearest bf16 -> float64 (the emulation's rounding points)."""
    return x.to(torch.float32).to(BF).to(torch.float64)


# ======================================================================================================================================
# Reference
# ======================================================================================================================================
class _Sec:
    """One row kind: exact float64 result, element bar, emulation and fp32 term, all shaped alike ((n, G, H, T, 64) for token rows, (n, H, 64) for CLS rows)."""

    def __init__(self, ref, bar, emu, F):
        self.ref, self.bar, self.emu, self.F = ref, bar, emu, F


def _core(Q, K, V, dO, scale, round_mid, cls=None):
    """All quantities of one batch of independent attention problems.  Q, dO: (B, Tq, 64); K, V: (B, nk, 64), float64.
    cls (the _clsq entry points): the LAST query row is the CLS query, whose probabilities on this group's keys (cls['p'], (B, nk)), delta (cls['delta'], exact;
    cls['delta_emu'], from the bf16 output row), u-level delta uncertainty (cls['ddelta']) and extra relative fp32 error of p (cls['relp']) are given.
    Returns exact dq (B, Tq, 64), dk, dv (B, nk, 64), the absolute sums A_*, the fp32 terms F_*, and the emulation e_* (before output rounding)."""
    aQ, aK, aV, aD = Q.abs(), K.abs(), V.abs(), dO.abs()
    nk, Tq = K.shape[1], Q.shape[1]
    s = scale * Q @ K.mT
    p = torch.softmax(s, -1)
    dp = dO @ V.mT
    if cls is not None:
        p[:, -1] = cls['p']
    delta = (p * dp).sum(-1)
    delta_e = delta.clone()
    if cls is not None:
        delta[:, -1] = cls['delta']
        delta_e[:, -1] = cls['delta_emu']
    ds = p * (dp - delta[..., None])
    dq, dk, dv = scale * ds @ K, scale * ds.mT @ Q, p.mT @ dO
    w = p * (dp.abs() + delta.abs()[..., None])
    A_dq, A_dk, A_dv = scale * w @ aK, scale * ds.abs().mT @ aQ, p.mT @ aD
    # fp32 terms
    ds_s = U32 * (66 * scale * (aQ @ aK.mT) + 2 * s.abs())                       # absolute error of a score = relative error of its exponential
    relp = ds_s + ds_s.amax(-1, keepdim=True) + (nk + 8) * U32                    # own score, the maximum's, the normaliser's sum
    if cls is not None:
        relp[:, -1] = ds_s[:, -1] + cls['relp'][:, None]                          # the statistics come from the forward
    ddp = 66 * U32 * (aD @ aV.mT)
    ddelta = (p * (ddp + relp * dp.abs())).sum(-1) + (nk + 2) * U32 * (p * dp.abs()).sum(-1)
    if cls is not None:
        ddelta[:, -1] = cls['ddelta'] + 66 * U32 * cls['ddelta'] / U              # u sum |dO o| (bf16 output row) + its 64-term fp32 dot
    E = p * (relp * (dp.abs() + delta.abs()[..., None]) + ddp + ddelta[..., None])   # absolute error of ds that is not a bf16 packing
    depth = (max(nk, Tq) + 16) * U32
    F_dq = scale * E @ aK + depth * A_dq
    F_dk = scale * E.mT @ aQ + depth * A_dk
    F_dv = (p * relp).mT @ aD + depth * A_dv
    ds_e = p * (dp - delta_e[..., None])
    if round_mid:
        e_dq = scale * (_rb(p * dp) @ K - delta_e[..., None] * (_rb(p) @ K))
        e_dk, e_dv = scale * _rb(ds_e).mT @ Q, _rb(p).mT @ dO
    else:
        e_dq, e_dk, e_dv = scale * ds_e @ K, scale * ds_e.mT @ Q, p.mT @ dO
        A_dq, A_dk, A_dv = torch.zeros_like(A_dq), torch.zeros_like(A_dk), torch.zeros_like(A_dv)
    return dict(dq=dq, dk=dk, dv=dv, A_dq=A_dq, A_dk=A_dk, A_dv=A_dv, F_dq=F_dq, F_dk=F_dk, F_dv=F_dv, e_dq=e_dq, e_dk=e_dk, e_dv=e_dv)


def _direct(ref, A, F, emu):
    """A row that the kernel stores itself: one bf16 rounding of its fp32 accumulator."""
    return _Sec(ref, MARGIN * (U * (A + ref.abs()) + F), _rb(emu), F)


def _reduced(ref_g, A_g, F_g, emu_g, G):
    """A row summed over the group axis (dim 1) from one bf16 partial per group by sf_reduce_groups_bf16 (fp32 sum, bf16 store)."""
    ref = ref_g.sum(1)
    sabs = ref_g.abs().sum(1)
    F = F_g.sum(1) + (G + 2) * U32 * sabs
    bar = MARGIN * (U * (A_g.sum(1) + sabs) + U * ref.abs() + F)
    return _Sec(ref, bar, _rb(_rb(emu_g).sum(1)), F)


def grouped_attention_bwd_ref(q, k, v, dO, geometry, scale, clsq=False, round_mid=True, fwd_packs_p=False):
    """float64 backward of the grouped attention of sf_attention: q, k, v, dO (n_seq, seq_rows, heads, 64) float64 (the bf16 inputs, widened);
    geometry = (n_groups, row0, group_stride, tok_stride, n_tok, cls_row).  Token t of group g is row row0 + g group_stride + t tok_stride and attends
    [CLS key (row cls_row, if >= 0); its group's tokens]; the CLS key's dk | dv is the sum over groups.  clsq: the CLS query attends every key of the sequence
    (the CLS key once).  round_mid: the kernel packs p / ds to bf16 before its second products (group kernel) or not (tiny kernel).  fwd_packs_p: the forward
    that produced the CLS query's output row packed its probabilities to bf16 before P V (attn_mfma_kernel; attn_tiny64_kernel and attn_cls64_kernel are fp32 up
    to the store), so that row carries u sum_k p_k |v_kd| besides its own rounding u |o_d|.
    Returns the sections dq_tok, dk_tok, dv_tok (n, G, H, T, 64), dk_cls, dv_cls, dq_cls (n, H, 64), `full` (dq, dk, dv as (n, seq_rows, H, 64), zero where
    nothing is written), the token row index (G, T), and for clsq the CLS query's log2-sum-exp `lse2` (n, H) and output row `o` (n, H, 64)."""
    n, R, H, _ = q.shape
    G, row0, gs, ts, T, cls_row = geometry
    has_cls = cls_row >= 0
    idx = row0 + torch.arange(G)[:, None] * gs + torch.arange(T)[None] * ts

    def grp(x):
        return x[:, idx].permute(0, 1, 3, 2, 4)                                   # (n, G, H, T, 64)

    Qg, Kg, Vg, Dg = grp(q), grp(k), grp(v), grp(dO)
    if has_cls:
        Kg = torch.cat([k[:, cls_row][:, None, :, None, :].expand(n, G, H, 1, 64), Kg], 3)
        Vg = torch.cat([v[:, cls_row][:, None, :, None, :].expand(n, G, H, 1, 64), Vg], 3)
    nk = T + (1 if has_cls else 0)
    out = {'idx': idx}
    cls = None
    if clsq:
        assert has_cls
        qc, dc = q[:, cls_row], dO[:, cls_row]                                    # (n, H, 64)
        Kall = torch.cat([k[:, cls_row][:, :, None], grp(k).permute(0, 2, 1, 3, 4).reshape(n, H, G * T, 64)], 2)
        Vall = torch.cat([v[:, cls_row][:, :, None], grp(v).permute(0, 2, 1, 3, 4).reshape(n, H, G * T, 64)], 2)
        sc = scale * torch.einsum('nhd,nhkd->nhk', qc, Kall)
        pc = torch.softmax(sc, -1)
        o = torch.einsum('nhk,nhkd->nhd', pc, Vall)
        out['lse2'], out['o'] = torch.logsumexp(sc, -1) * LOG2E, o
        pg = torch.zeros(n, G, H, nk, dtype=torch.float64, device=q.device)
        pg[:, 0, :, 0] = pc[..., 0]                                               # the CLS key counts for the CLS query in group 0 only
        pg[..., 1:] = pc[..., 1:].reshape(n, H, G, T).permute(0, 2, 1, 3)
        bc = lambda x: x[:, None].expand(n, G, *x.shape[1:]).reshape(n * G * H, *x.shape[2:])   # noqa: E731
        nall = 1 + G * T
        # the forward's (M, L) in fp32: M exact up to its conversion to the base-2 domain, L an n-term fp32 sum of exponentials (worst case: one chain)
        relp = U32 * (2 * sc.abs().amax(-1) + 2 * out['lse2'].abs() + nall + 16)
        o_abs, o_emu = o.abs(), _rb(o)
        if fwd_packs_p:
            o_abs = o_abs + torch.einsum('nhk,nhkd->nhd', pc, Vall.abs())
            o_emu = _rb(torch.einsum('nhk,nhkd->nhd', _rb(pc), Vall))
        cls = dict(p=pg.reshape(n * G * H, nk), delta=bc((dc * o).sum(-1)), delta_emu=bc((dc * o_emu).sum(-1)), ddelta=bc(U * (dc.abs() * o_abs).sum(-1)), relp=bc(relp))
        Qg = torch.cat([Qg, qc[:, None, :, None, :].expand(n, G, H, 1, 64)], 3)
        Dg = torch.cat([Dg, dc[:, None, :, None, :].expand(n, G, H, 1, 64)], 3)
    B = n * G * H
    c = _core(Qg.reshape(B, -1, 64), Kg.reshape(B, nk, 64), Vg.reshape(B, nk, 64), Dg.reshape(B, -1, 64), scale, round_mid, cls)
    c = {key: val.reshape(n, G, H, -1, 64) for key, val in c.items()}
    c0 = 1 if has_cls else 0
    out['dq_tok'] = _direct(c['dq'][..., :T, :], c['A_dq'][..., :T, :], c['F_dq'][..., :T, :], c['e_dq'][..., :T, :])
    out['dk_tok'] = _direct(c['dk'][..., c0:, :], c['A_dk'][..., c0:, :], c['F_dk'][..., c0:, :], c['e_dk'][..., c0:, :])
    out['dv_tok'] = _direct(c['dv'][..., c0:, :], c['A_dv'][..., c0:, :], c['F_dv'][..., c0:, :], c['e_dv'][..., c0:, :])
    full = {x: torch.zeros(n, R, H, 64, dtype=torch.float64, device=q.device) for x in ('dq', 'dk', 'dv')}
    for x in ('dq', 'dk', 'dv'):
        full[x][:, idx] = out[x + '_tok'].ref.permute(0, 1, 3, 2, 4)
    if has_cls:
        for x in ('dk', 'dv'):
            out[x + '_cls'] = _reduced(c[x][..., 0, :], c['A_' + x][..., 0, :], c['F_' + x][..., 0, :], c['e_' + x][..., 0, :], G)
            full[x][:, cls_row] = out[x + '_cls'].ref
    if clsq:
        out['dq_cls'] = _reduced(c['dq'][..., T, :], c['A_dq'][..., T, :], c['F_dq'][..., T, :], c['e_dq'][..., T, :], G)
        full['dq'][:, cls_row] = out['dq_cls'].ref
    out['full'] = full
    # the emulated per-group partial rows (n, G, H, 64) behind the reduced sections, before their own bf16 rounding (tower_bwd_oracle's group-sum plants)
    out['partials'] = {x: c['e_' + x][..., 0, :] for x in ('dk', 'dv')} if has_cls else {}
    if clsq:
        out['partials']['dq'] = c['e_dq'][..., T, :]
    return out


def _forward_autograd(q, k, v, geometry, scale, clsq):
    """The forward written independently of the helper above (loops over groups), for autograd: (n, seq_rows, H, 64) with zeros on rows that have no query."""
    n, R, H, _ = q.shape
    G, row0, gs, ts, T, cls_row = geometry
    rows = {}
    for g in range(G):
        tok = [row0 + g * gs + t * ts for t in range(T)]
        keys = ([cls_row] if cls_row >= 0 else []) + tok
        s = scale * torch.einsum('nthd,nkhd->nhtk', q[:, tok], k[:, keys])
        o = torch.einsum('nhtk,nkhd->nthd', torch.softmax(s, -1), v[:, keys])
        for j, r in enumerate(tok):
            rows[r] = o[:, j]
    if clsq:
        keys = [cls_row] + [row0 + g * gs + t * ts for g in range(G) for t in range(T)]
        s = scale * torch.einsum('nhd,nkhd->nhk', q[:, cls_row], k[:, keys])
        rows[cls_row] = torch.einsum('nhk,nkhd->nhd', torch.softmax(s, -1), v[:, keys])
    zero = torch.zeros(n, H, 64, dtype=torch.float64, device=q.device)
    return torch.stack([rows.get(r, zero) for r in range(R)], 1)
