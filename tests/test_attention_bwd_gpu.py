"""GPU: the attention backward kernels of both trainers (csrc/sf_attention.hip, csrc/sf_towerbwd.hip, csrc/sf_train.hip) element by element against a float64
restatement of the same operation, computed on the host from the very bf16-rounded inputs the kernel sees, at the tile, group and argument edges of the launchers.

Reference (grouped_attention_bwd_ref): s = scale q k^T, p = softmax(s), dp = dO v^T, delta = sum_k p dp, ds = p (dp - delta), dq = scale ds k, dk = scale ds^T q,
dv = p^T dO, with the group geometry of the ABI; it lives in tests/attention_bwd_oracle.py and is checked against float64 autograd on the CPU
(tests/test_tower_bwd_oracle_cpu.py::test_attention_bwd_reference_matches_float64_autograd).

Bars.  u = 2^-8 (bf16), e = 2^-24 (fp32).  For every written element  |got - ref| <= 1.5 * (u * (A + |ref|) + F), where
  A  is the first-order worst case of the bf16 roundings INSIDE the kernel (read from the kernel, stated per test), as sums of absolute values:
       dq[i,d]: scale sum_k p_ik (|dp_ik| + |delta_i|) |k_kd|     (attn_group_bwd_kernel packs e and e*dp to bf16 before the dQ MFMAs, delta stays fp32)
       dk[j,d]: scale sum_i |ds_ij| |q_id|                         (p (dp - delta) packed to bf16 before the dK MFMA)
       dv[j,d]: sum_i p_ij |dO_id|                                 (p packed to bf16 before the dV MFMA)
     kernels that are fp32 up to their stores (attn_tiny64_bwd_kernel: ds and p cross LDS as fp32; attention_cls_bwd_kernel) have A = 0;
  u |ref| is the bf16 rounding of the output itself;
  F  is the fp32 term, never zero: the score's 64-term dot (66 e scale sum_d |q_d k_d|) and the exponent's argument (2 e |s|) as a relative error of p, the
     normaliser ((nk + 8) e), the 64-term dot of dp and the nk-term sum of delta seen through the cancellation dp - delta, and (n + 16) e times the absolute sums
     of the output's own accumulation.  With one key ds is mathematically 0, the u-terms of dk vanish and F alone is the bar.
  Rows that are summed over groups (the CLS key's dk | dv, the CLS query's dq of the _clsq entry points) go through one bf16 partial per group and
  sf_reduce_groups_bf16: the bar is the sum of the groups' bars (each with u |partial_g|) + u |sum| + G e sum_g |partial_g|.
  For _clsq the CLS query's delta is <dO, o> with the forward's bf16 output row: u sum_d |dO_d o_d| (and, where that forward is attn_mfma_kernel, which packs its
  probabilities to bf16 before P V, u sum_d |dO_d| sum_k p_k |v_kd|) enters ds of that query as p_ck times that, and its probabilities carry the fp32 error of
  the forward's statistics (M, L).
  The factor 1.5 is the one common margin for second-order terms and v_exp_f32.
Statistical criterion.  Per (sequence, head, row kind) with at least 64 elements: ||got - ref||_2 <= 2 ||emu - ref||_2 + ||F||_2, where emu is a float64 emulation
that rounds to bf16 at the points listed above (and at the outputs / partials).  The factor 2 covers that the kernel's roundings are other draws of the same
distribution; ||F||_2 keeps the threshold above zero where the emulation is exact (one key: ds = 0).  Both sides come from the reference and the emulation only.

Every comparison covers all written elements; outputs are pre-filled with a bf16 canary pattern and must be bit-equal wherever the kernel must not write."""
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attention_bwd_oracle import (BF, LOG2E, MARGIN, U, U32, _core, _direct, _rb, _reduced, _Sec,  # noqa: E402,F401
                                  grouped_attention_bwd_ref)

STAT_FACTOR = 2.0


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


def _bf16_ulp(ref):
    a = ref.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


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
# Comparison
# ======================================================================================================================================
WORST = {}                 # kernel -> worst observed error / bar ratio (printed per test, collected by the report at the end of the module)


def _check_section(kernel, kind, got, sec, key_shift=0, stat=True):
    """Element bar over every element of the section, then the statistical criterion per (sequence, head).  Returns the worst error / bar ratio."""
    err = (got - sec.ref).abs()
    ratio = err / sec.bar
    worst = ratio.max().item() if ratio.numel() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst if math.isfinite(worst) else float('inf'))
    print(f'{kernel} {kind}: worst err / bar {worst:.3f} over {ratio.numel()} elements')
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
            WORST[kernel + ' (rel-L2 / threshold)'] = max(WORST.get(kernel + ' (rel-L2 / threshold)', 0.0), worst_stat)
            if not (e <= thr).all():
                s_, h_ = _unravel(torch.nan_to_num(r, nan=float('inf')).flatten().argmax().item(), r.shape)
                nrm = l2(sec.ref)[s_, h_].item()
                raise AssertionError(f'{kernel} {kind}: sequence {s_} head {h_}: rel-L2 error {e[s_, h_].item() / max(nrm, 1e-300):.3g} above '
                                     f'{thr[s_, h_].item() / max(nrm, 1e-300):.3g} = 2 x the bf16 emulation\'s distance (+ fp32 term); ratio {r[s_, h_].item():.3g}, '
                                     f'worst element err / bar {worst:.3g}')
    return worst, worst_stat


class _Case:
    """Host and device buffers of one grouped-attention backward launch.  q | k | v are column blocks of one (rows, ld) buffer, dq | dk | dv of one (rows, ldg)
    canary-filled buffer; strides wider than the data by pad_* elements."""

    def __init__(self, gpu, n, G, H, T, cls, layout='group_major', row0=None, cls_row=None, extra_rows=2, pad=(0, 0, 0), seed=0, mode='normal', peak='first'):
        self.n, self.G, self.H, self.T = n, G, H, T
        if cls_row is None:
            cls_row = 0 if cls else -1
        if row0 is None:
            row0 = 1 if cls_row == 0 else 0
        gs, ts = (T, 1) if layout == 'group_major' else (1, G)
        self.geo = (G, row0, gs, ts, T, cls_row)
        self.R = R = max(row0 + (G - 1) * gs + (T - 1) * ts, cls_row) + 1 + extra_rows
        self.Hd = Hd = H * 64
        self.ld, self.lddo, self.ldg = 3 * Hd + pad[0], Hd + pad[1], 3 * Hd + pad[2]
        g = _gen(1000 + seed)
        qkv = torch.randn(n * R, self.ld, generator=g) * 0.8
        dO = torch.randn(n * R, self.lddo, generator=g) * 0.5
        idx = row0 + torch.arange(G)[:, None] * gs + torch.arange(T)[None] * ts
        v4 = qkv.view(n, R, self.ld)
        nk = T + (1 if cls_row >= 0 else 0)
        if mode == 'sharp':
            # every query is 6 x one key of its group (p ~ 1 there); that key sits in the first, a middle or the last key tile
            nkt = (nk + 15) // 16
            t0 = {'first': 0, 'middle': (nkt // 2) * 16, 'last': (nkt - 1) * 16}[peak]
            span = min(16, nk - t0)
            for gi in range(G):
                for t in range(T):
                    j = t0 + t % span                                             # key slot in [CLS; tokens]
                    krow = cls_row if (cls_row >= 0 and j == 0) else int(idx[gi, j - (1 if cls_row >= 0 else 0)])
                    v4[:, int(idx[gi, t]), :Hd] = 6 * v4[:, krow, Hd:2 * Hd].to(BF).float()
        elif mode == 'negative':
            # every score is about -5: keys share a component c (|c|^2 ~ 41), queries are -c + noise.  A key slot beyond n_tok (a zero row, score 0) that a wrong
            # mask lets into the softmax then outweighs the real keys instead of adding 1 / nk to the normaliser
            cvec = torch.randn(Hd, generator=g) * 0.8
            v4[:, :, Hd:2 * Hd] = cvec + 0.3 * v4[:, :, Hd:2 * Hd]
            v4[:, :, :Hd] = -cvec + v4[:, :, :Hd]
        elif mode == 'flat':
            v4[:, :, Hd:2 * Hd] = v4[:, :1, Hd:2 * Hd]                           # all keys equal: p = 1 / nk
        elif mode == 'cls_key_dominant':
            v4[:, cls_row, :Hd] = 6 * v4[:, cls_row, Hd:2 * Hd].to(BF).float()   # the CLS query is 6 x the CLS key
        elif mode == 'cls_key_half':
            # the CLS query is alpha x the CLS key, alpha per (sequence, head) by bisection on the float64 softmax so that the CLS key holds half of the CLS
            # query's probability: p = 1 would make ds of that key vanish (dp = delta), p = 1/2 makes its share of dq and dk as large as it can be
            kc = v4[:, cls_row, Hd:2 * Hd].to(BF).double().view(n, H, 64)
            kt = v4[:, idx.flatten(), Hd:2 * Hd].to(BF).double().view(n, -1, H, 64)
            a_cls, a_tok = 0.125 * (kc * kc).sum(-1), 0.125 * torch.einsum('nhd,nkhd->nhk', kc, kt)
            lo, hi = torch.zeros(n, H, dtype=torch.float64), torch.full((n, H), 16.0, dtype=torch.float64)
            for _ in range(40):
                mid = (lo + hi) / 2
                above = mid * a_cls > torch.logsumexp(mid[..., None] * a_tok, -1)     # p_cls > 1/2
                lo, hi = torch.where(above, lo, mid), torch.where(above, mid, hi)
            v4[:, cls_row, :Hd] = (hi[..., None] * kc).reshape(n, Hd).float()
        self.qkv_h, self.dO_h = qkv.to(BF), dO.to(BF)
        self.qkv, self.dO = self.qkv_h.to(gpu), self.dO_h.to(gpu)
        self.canary = _canary(n * R, self.ldg, seed)
        self.d = self.canary.clone().to(gpu)
        self.part_canary = _canary(n * G, 2 * Hd, seed + 1)
        self.part = self.part_canary.clone().to(gpu)
        self.dqc = _canary(n * G, Hd, seed + 2).to(gpu)
        self.gpu, self.idx, self.cls_row = gpu, idx, cls_row

    def wide(self):
        n, R, H, Hd = self.n, self.R, self.H, self.Hd
        x = self.qkv_h.double().view(n, R, self.ld)
        return (x[..., :Hd].reshape(n, R, H, 64), x[..., Hd:2 * Hd].reshape(n, R, H, 64), x[..., 2 * Hd:3 * Hd].reshape(n, R, H, 64),
                self.dO_h.double().view(n, R, self.lddo)[..., :Hd].reshape(n, R, H, 64))

    def head_args(self):
        Hd, d = self.Hd, self.d
        return (self.qkv.data_ptr(), self.qkv[:, Hd:].data_ptr(), self.qkv[:, 2 * Hd:].data_ptr(), self.ld, self.dO.data_ptr(), self.lddo, d.data_ptr(),
                d[:, Hd:].data_ptr(), d[:, 2 * Hd:].data_ptr(), self.ldg, self.part.data_ptr())

    def tail_args(self, scale=0.125):
        return (self.n, self.R, *self.geo, self.H, 64, scale, _st())

    def reduce(self, clsq):
        """The trainer's reductions of the per-group partials into the CLS row of dk | dv (and dq)."""
        n, G, Hd, R, d = self.n, self.G, self.Hd, self.R, self.d
        if self.cls_row >= 0:
            _ok(_lib().sf_reduce_groups_bf16(self.part.data_ptr(), G * 2 * Hd, 2 * Hd, G, d[self.cls_row:, Hd:].data_ptr(), R * self.ldg, 2 * Hd, n, 0, _st()), 'reduce dk|dv')
        if clsq:
            _ok(_lib().sf_reduce_groups_bf16(self.dqc.data_ptr(), G * Hd, Hd, G, d[self.cls_row:].data_ptr(), R * self.ldg, Hd, n, 0, _st()), 'reduce dq')

    def forward_stats(self, scale=0.125, via='combine'):
        """The forward as the trainer runs it: attention output + the CLS query's merged statistics (sf_attention_cls_partial + sf_attention_cls_combine_stats), or
        sf_attention_cls_stats over all keys of the sequence (rows cls_row .. cls_row + G T, contiguous in both layouts with cls_row = 0, row0 = 1)."""
        n, R, H, Hd, G, T = self.n, self.R, self.H, self.Hd, self.G, self.T
        att = torch.zeros(n * R, Hd, device=self.gpu, dtype=BF)
        stats = torch.empty(n * H * 2, device=self.gpu)
        q, k, v = self.qkv, self.qkv[:, Hd:], self.qkv[:, 2 * Hd:]
        if via == 'combine':
            fpart = torch.empty(n * H * G * 66, device=self.gpu)
            _ok(_lib().sf_attention_cls_partial(q.data_ptr(), k.data_ptr(), v.data_ptr(), self.ld, att.data_ptr(), Hd, n, R, *self.geo, H, 64, scale, fpart.data_ptr(), _st()),
                'sf_attention_cls_partial')
            _ok(_lib().sf_attention_cls_combine_stats(fpart.data_ptr(), G, att.data_ptr(), Hd, R, self.cls_row, n, H, stats.data_ptr(), _st()), 'sf_attention_cls_combine_stats')
        else:
            assert self.cls_row == 0 and self.geo[1] == 1
            _ok(_lib().sf_attention_cls_stats(q.data_ptr(), R, 0, k.data_ptr(), v.data_ptr(), self.ld, R, 0, 1 + G * T, att.data_ptr(), Hd, R, 0, n, H, 64, scale,
                                              stats.data_ptr(), _st()), 'sf_attention_cls_stats')
        return att, stats

    def compare(self, kernel, ref, clsq):
        torch.cuda.synchronize()
        n, R, H, Hd, T = self.n, self.R, self.H, self.Hd, self.T
        raw = self.d.cpu()
        got = raw.double().view(n, R, self.ldg)
        blk = lambda i: got[..., i * Hd:(i + 1) * Hd].reshape(n, R, H, 64)         # noqa: E731
        tok = lambda x: x[:, self.idx].permute(0, 1, 3, 2, 4)                       # noqa: E731
        c0 = 1 if self.cls_row >= 0 else 0
        res, failed = {}, []

        def section(key, kind, got_, **kw):                                        # every row kind is checked and reported, not only the first that fails
            try:
                res[key] = _check_section(kernel, kind, got_, ref[key], **kw)
            except AssertionError as e:
                failed.append(f'[{key}] {e}')

        for i, name in enumerate(('dq', 'dk', 'dv')):
            section(name + '_tok', f'{name} of the token rows', tok(blk(i)), key_shift=c0 if i else 0)
        if self.cls_row >= 0:
            for i, name in ((1, 'dk'), (2, 'dv')):
                section(name + '_cls', f'{name} of the CLS key', blk(i)[:, self.cls_row])
        if clsq:
            section('dq_cls', 'dq of the CLS query', blk(0)[:, self.cls_row])
        assert not failed, f'{len(failed)} row kinds outside their bars: ' + ' || '.join(failed)
        written = torch.zeros(n, R, self.ldg, dtype=torch.bool)
        written[:, self.idx.flatten(), :3 * Hd] = True
        if self.cls_row >= 0:
            written[:, self.cls_row, (0 if clsq else Hd):3 * Hd] = True
        _assert_untouched(raw, self.canary, written.view(n * R, self.ldg), f'{kernel}: d(q|k|v)')
        return res


def _run_group(gpu, kernel='group', clsq=False, scale=0.125, stats_via='combine', **kw):
    """One launch of sf_attention_group_bwd[_clsq] / sf_attention_tiny_bwd[_clsq] + the reductions, compared with float64.  Returns the per-section ratios."""
    c = _Case(gpu, **kw)
    name = f'sf_attention_{kernel}_bwd' + ('_clsq' if clsq else '')
    fn = getattr(_lib(), name)
    if clsq:
        att, stats = c.forward_stats(scale, stats_via)
        _ok(fn(*c.head_args(), stats.data_ptr(), att.data_ptr(), c.Hd, c.dqc.data_ptr(), *c.tail_args(scale)), name)
    else:
        _ok(fn(*c.head_args(), *c.tail_args(scale)), name)
    c.reduce(clsq)
    q, k, v, dO = c.wide()
    ref = grouped_attention_bwd_ref(q, k, v, dO, c.geo, scale, clsq=clsq, round_mid=(kernel == 'group'),
                                    fwd_packs_p=(clsq and stats_via == 'combine' and c.T > 8))      # sf_attention_cls_partial: n_tok > 8 runs attn_mfma_kernel
    res = c.compare(name, ref, clsq)
    if clsq:                                                                        # the statistics the backward ran on
        st = stats.cpu().double().view(c.n, c.H, 2)
        assert c.cls_row == 0 and c.geo[1] == 1
        _check_lse2(name + ' statistics', st, ref['lse2'], q[:, 0], k[:, :1 + c.G * c.T], scale)
    print(f'{name} {kw}: ' + ', '.join(f'{x} {a:.3f}/{b:.3f}' for x, (a, b) in res.items()))
    return res


def _check_lse2(what, st, lse2, qc, keys, scale):
    """(m, l) of a CLS query (qc (n, H, 64)) over keys (n, n_keys, H, 64) against float64: m is the maximum in the base-2 domain, max_j s_j log2 e, and
    m + log2 l = log2 sum_j exp(s_j) is what the backward uses.  fp32 bars, in the base-2 domain: the scores' 64-term dots (66 e scale max_j sum_d |q_d k_jd|) and
    the conversions of m (4 e |m|) for m; for m + log2 l in addition l as a sum of n_keys exponentials (worst case one chain: (n_keys + 16) e relative) whose
    arguments s_j - m carry 2 e (|m| + |lse|)."""
    n_keys = keys.shape[1]
    s2max = (scale * torch.einsum('nhd,nrhd->nhr', qc, keys)).amax(-1) * LOG2E
    amax = torch.einsum('nhd,nrhd->nhr', qc.abs(), keys.abs()).amax(-1)
    mbar = MARGIN * U32 * (66 * scale * amax * LOG2E + 4 * s2max.abs())
    assert torch.isfinite(st).all() and (st[..., 1] >= 1.0 - 1e-3).all(), f'{what}: l < 1 or not finite'
    merr = (st[..., 0] - s2max).abs()
    assert (merr <= mbar).all(), f'{what}: m is not the base-2 maximum: off by {merr.max().item():.3g} (bar {mbar.min().item():.3g})'
    got = st[..., 0] + torch.log2(st[..., 1])
    bar = mbar + MARGIN * U32 * LOG2E * (2 * s2max.abs() / LOG2E + 2 * lse2.abs() / LOG2E + n_keys + 16)
    err = (got - lse2).abs()
    WORST[what] = max(WORST.get(what, 0.0), (err / bar).max().item())
    assert (err <= bar).all(), f'{what}: m + log2 l off by {err.max().item():.3g} (bar {bar.min().item():.3g}, worst ratio {(err / bar).max().item():.3g})'
    return got, bar


# ======================================================================================================================================
# 1. sf_attention_group_bwd (attn_group_bwd_kernel<16, true>; <8, false> and <16, false> through the measurement hooks)
# ======================================================================================================================================
SWEEP_CLS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 74, 111, 112, 113, 191, 192, 193, 196, 207]
SWEEP_NOCLS = [1, 16, 17, 32, 33, 74, 208]


@pytest.mark.gpu
@pytest.mark.parametrize('n_tok,cls', [(t, True) for t in SWEEP_CLS] + [(t, False) for t in SWEEP_NOCLS])
def test_group_bwd_tile_sweep(gpu, n_tok, cls):
    """The 16-row tiles walked in pairs: a missing odd tile (zero half), the (kt + 2) * 16 > nk key mask, nqt != nkt (n_tok % 16 == 0 with a CLS key), one key.
    Rounding points of attn_group_bwd_kernel: e and e * dp packed to bf16 before the dQ MFMAs (delta, l in fp32), p and p (dp - delta) packed before the dV / dK MFMAs,
    bf16 stores; the CLS key's dk | dv as one bf16 partial per group + sf_reduce_groups_bf16.  Each shape runs on N(0, 0.8) inputs and on inputs whose scores are
    all about -5 (mode 'negative' of _Case): there a masked key slot that leaks into the softmax (score 0) dominates it, at any n_tok."""
    _run_group(gpu, n=1, G=2, H=2, T=n_tok, cls=cls, seed=n_tok)
    _run_group(gpu, n=1, G=2, H=2, T=n_tok, cls=cls, seed=n_tok, mode='negative')


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [
    dict(n=3, G=3, H=5, T=33, cls=True, layout='tok_major', pad=(8, 16, 24)),
    dict(n=1, G=8, H=12, T=17, cls=True, layout='group_major', pad=(0, 8, 0)),
    dict(n=3, G=8, H=1, T=49, cls=True, layout='tok_major', pad=(16, 0, 8)),
    dict(n=1, G=3, H=5, T=74, cls=False, layout='tok_major', row0=1, pad=(8, 8, 8)),
    dict(n=3, G=1, H=12, T=74, cls=False, layout='group_major', row0=0),
    dict(n=1, G=3, H=1, T=20, cls=True, cls_row=3 * 20 + 1, row0=0, layout='group_major', pad=(8, 0, 16)),        # the CLS row behind the groups
    dict(n=3, G=8, H=5, T=5, cls=True, cls_row=2, row0=4, layout='tok_major', extra_rows=3),                        # ... and between unused rows
    dict(n=1, G=1, H=12, T=196, cls=True, layout='group_major', pad=(8, 8, 8)),
], ids=lambda kw: '-'.join(f'{k}{v}' for k, v in kw.items() if k in ('n', 'G', 'H', 'T', 'layout')))
def test_group_bwd_layouts(gpu, kw):
    """Both memory layouts of the trainers (group_stride = n_tok, tok_stride = 1 and group_stride = 1, tok_stride = n_groups), row0 0 / 1 / 4, a CLS row that is
    not row 0, n_groups 1 / 3 / 8, heads 1 / 5 / 12, n_seq 1 / 3, ld / lddo / ldg wider than the data; rows outside every group and padding columns keep their canary."""
    _run_group(gpu, seed=7, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', [33, 196])
@pytest.mark.parametrize('mode,peak', [('sharp', 'first'), ('sharp', 'middle'), ('sharp', 'last'), ('flat', 'first')])
def test_group_bwd_sharp_and_flat_softmax(gpu, n_tok, mode, peak):
    """Queries 6 x one key (p ~ 1 on it) with that key in the first, a middle or the last key tile - the running maximum of the online softmax moves late, early or
    never (the m_new != m rescale) - and all keys equal (p = 1 / nk, no rescale after the first tile)."""
    _run_group(gpu, n=1, G=2, H=2, T=n_tok, cls=True, mode=mode, peak=peak, seed=11)


@pytest.mark.gpu
def test_group_bwd_rejects_209_rows(gpu):
    c = _Case(gpu, n=1, G=1, H=1, T=208, cls=True)
    _rejected(_lib().sf_attention_group_bwd(*c.head_args(), *c.tail_args()), 'n_tok + cls = 209')
    c = _Case(gpu, n=1, G=1, H=1, T=209, cls=False)
    _rejected(_lib().sf_attention_group_bwd(*c.head_args(), *c.tail_args()), 'n_tok = 209')
    torch.cuda.synchronize()
    assert torch.equal(c.d.cpu().view(torch.int16), c.canary.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize('var,value', [('SF_GB_WAVES', '8'), ('SF_GB_X32', '0')])
def test_group_bwd_measurement_hooks(gpu, var, value):
    """attn_group_bwd_kernel<8, false> (SF_GB_WAVES=8) and <16, false> (SF_GB_X32=0) ship in the product library: the tile sweep once more under each, in a fresh
    child process (the launcher reads the variables once per process)."""
    assert 'SF_GB_WAVES' not in os.environ and 'SF_GB_X32' not in os.environ, 'the measurement hooks must not be set for this suite'
    env = dict(os.environ)
    env[var] = value
    here = Path(__file__).resolve()
    r = subprocess.run([sys.executable, '-m', 'pytest', str(here), '-q', '-x', '-p', 'no:cacheprovider', '-k', 'test_group_bwd_tile_sweep'], env=env, cwd=str(here.parent.parent),
                       capture_output=True, text=True, timeout=300)
    tail = '\n'.join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0, f'{var}={value}: exit status {r.returncode}\n{tail}'
    assert f'{len(SWEEP_CLS) + len(SWEEP_NOCLS)} passed' in r.stdout, tail


# ======================================================================================================================================
# 2. sf_attention_group_bwd_clsq
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', [1, 15, 17, 31, 33, 195, 196, 207])
@pytest.mark.parametrize('layout', ['group_major', 'tok_major'])
def test_group_bwd_clsq(gpu, n_tok, layout):
    """All rows against float64: the CLS query's dq (one bf16 partial per group + sf_reduce_groups_bf16), every dk | dv (token rows now include the CLS query's
    share), the token rows' dq.  Statistics from sf_attention_cls_partial + sf_attention_cls_combine_stats as the trainer does, checked against float64 themselves.
    Extra rounding point: delta of the CLS query is <dO, o> with the forward's bf16 output row."""
    _run_group(gpu, clsq=True, n=1, G=3, H=2, T=n_tok, cls=True, layout=layout, seed=n_tok)


@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', [17, 196])
@pytest.mark.parametrize('mode', ['cls_key_dominant', 'cls_key_half'])
def test_group_bwd_clsq_cls_key_counts_once(gpu, n_tok, mode):
    """The CLS key counts for the CLS query in group 0 only.  'dominant': the CLS query is 6 x the CLS key, p ~ 1 on it - counted in every group, the CLS key's dv
    would be n_groups times too large (its ds vanishes: dp = delta).  'half': the CLS key holds half of the CLS query's probability, so the CLS query's dq and the
    CLS key's dk would be wrong as well."""
    res = _run_group(gpu, clsq=True, n=2, G=3, H=2, T=n_tok, cls=True, mode=mode, seed=5)
    assert 'dq_cls' in res


@pytest.mark.gpu
def test_group_bwd_clsq_statistics_paths_agree(gpu):
    """sf_attention_cls_stats over all keys and sf_attention_cls_partial + sf_attention_cls_combine_stats give the same m + log2 l within the fp32 bar, and the
    backward on either is within the bars."""
    _run_group(gpu, clsq=True, stats_via='cls_stats', n=2, G=8, H=2, T=33, cls=True, seed=9)
    _run_group(gpu, clsq=True, stats_via='cls_stats', n=1, G=2, H=12, T=196, cls=True, layout='tok_major', seed=9)


@pytest.mark.gpu
def test_group_bwd_clsq_rejections(gpu):
    c = _Case(gpu, n=1, G=2, H=1, T=16, cls=True)
    att = torch.zeros(c.n * c.R, c.Hd, device=gpu, dtype=BF)
    stats = torch.ones(2, device=gpu)
    fn = _lib().sf_attention_group_bwd_clsq
    _rejected(fn(*c.head_args(), stats.data_ptr(), att.data_ptr(), c.Hd, c.dqc.data_ptr(), *c.tail_args()), 'n_tok % 16 == 0')
    c = _Case(gpu, n=1, G=2, H=1, T=17, cls=True)
    att = torch.zeros(c.n * c.R, c.Hd, device=gpu, dtype=BF)
    _rejected(fn(*c.head_args(), None, att.data_ptr(), c.Hd, c.dqc.data_ptr(), *c.tail_args()), 'no statistics')
    torch.cuda.synchronize()
    assert torch.equal(c.d.cpu().view(torch.int16), c.canary.view(torch.int16))


# ======================================================================================================================================
# 3. sf_attention_tiny_bwd / sf_attention_tiny_bwd_clsq
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', range(1, 9))
@pytest.mark.parametrize('cls', [True, False])
@pytest.mark.parametrize('n,G,H', [(1, 1, 1), (1, 5, 1), (2, 2, 3), (1, 13, 1)], ids=['units1', 'units5', 'units12', 'units13'])
def test_tiny_bwd(gpu, n_tok, cls, n, G, H):
    """attn_tiny64_bwd_kernel: fp32 up to its stores (ds and p cross LDS as fp32), so A = 0 and the bar is u |ref| + F (+ the partial / reduction terms of the CLS
    key).  One wave per unit, four units per workgroup: 1, 5, 4k and 4k + 1 units; idle query lanes (n_tok < 8) re-read the last token and must add nothing."""
    _run_group(gpu, kernel='tiny', n=n, G=G, H=H, T=n_tok, cls=cls, layout='tok_major' if G > 1 else 'group_major', seed=n_tok, pad=(8, 0, 8))


@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', range(1, 9))
@pytest.mark.parametrize('n,G,H', [(1, 1, 1), (1, 5, 1), (2, 2, 3), (1, 13, 1)], ids=['units1', 'units5', 'units12', 'units13'])
def test_tiny_bwd_clsq(gpu, n_tok, n, G, H):
    """The CLS query as a ninth query of every group, on the statistics of sf_attention_cls_stats over all keys (the Stage-1 trainer's path)."""
    _run_group(gpu, kernel='tiny', clsq=True, stats_via='cls_stats', n=n, G=G, H=H, T=n_tok, cls=True, layout='tok_major', seed=n_tok)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['cls_key_dominant', 'cls_key_half'])
def test_tiny_bwd_clsq_cls_key_counts_once(gpu, mode):
    _run_group(gpu, kernel='tiny', clsq=True, stats_via='cls_stats', n=2, G=5, H=2, T=8, cls=True, layout='tok_major', mode=mode, seed=5)


@pytest.mark.gpu
def test_tiny_bwd_rejects_9_tokens(gpu):
    c = _Case(gpu, n=1, G=1, H=1, T=9, cls=True)
    _rejected(_lib().sf_attention_tiny_bwd(*c.head_args(), *c.tail_args()), 'n_tok = 9')
    att = torch.zeros(c.n * c.R, c.Hd, device=gpu, dtype=BF)
    stats = torch.ones(2, device=gpu)
    _rejected(_lib().sf_attention_tiny_bwd_clsq(*c.head_args(), stats.data_ptr(), att.data_ptr(), c.Hd, c.dqc.data_ptr(), *c.tail_args()), 'n_tok = 9 (clsq)')
    torch.cuda.synchronize()
    assert torch.equal(c.d.cpu().view(torch.int16), c.canary.view(torch.int16))


# ======================================================================================================================================
# 4. sf_attention_cls_bwd
# ======================================================================================================================================
def _cls_bwd_case(gpu, n_keys, H, n=2, q_row=0, kv_row0=0, do_row=0, extra=0, accumulate=0, mode='normal', seed=0):
    R = max(kv_row0 + n_keys + extra, q_row + 1)
    Rdo = do_row + 2
    Hd = H * 64
    ld, lddo, ldg = 3 * Hd + 8, Hd + 8, 3 * Hd + 16
    g = _gen(2000 + seed)
    qkv = torch.randn(n * R, ld, generator=g) * 0.8
    if mode == 'sharp':
        qkv.view(n, R, ld)[:, q_row, :Hd] = 6 * qkv.view(n, R, ld)[:, kv_row0 + n_keys // 2, Hd:2 * Hd].to(BF).float()
    qkv = qkv.to(BF)
    dO = (torch.randn(n * Rdo, lddo, generator=g) * 0.5).to(BF)
    pre = (torch.randn(n * R, ldg, generator=g) * 0.3 + 2.0).to(BF)                # non-zero prefill: the accumulate operand and the canary at once
    d = pre.clone().to(gpu)
    qd, dod = qkv.to(gpu), dO.to(gpu)
    rc = _lib().sf_attention_cls_bwd(qd.data_ptr(), R, q_row, qd[:, Hd:].data_ptr(), qd[:, 2 * Hd:].data_ptr(), ld, R, kv_row0, n_keys, dod.data_ptr(), lddo, Rdo, do_row,
                                     d.data_ptr(), d[:, Hd:].data_ptr(), d[:, 2 * Hd:].data_ptr(), ldg, n, H, 64, 0.125, accumulate, _st())
    return rc, dict(n=n, R=R, Rdo=Rdo, H=H, Hd=Hd, ld=ld, lddo=lddo, ldg=ldg, qkv=qkv, dO=dO, pre=pre, d=d)


@pytest.mark.gpu
@pytest.mark.parametrize('n_keys', [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1569, 2048])
@pytest.mark.parametrize('H,accumulate,rows', [(1, 0, (0, 0, 0, 0)), (12, 1, (0, 0, 0, 0)), (1, 1, (2, 3, 1, 5)), (12, 0, (5, 1, 1, 2))],
                         ids=['h1-overwrite', 'h12-accumulate', 'h1-accumulate-offsets', 'h12-overwrite-offsets'])
def test_cls_bwd(gpu, n_keys, H, accumulate, rows):
    """attention_cls_bwd_kernel is fp32 throughout and rounds only its stores: bar = 1.5 (u |ref| + F).  64 keys per sweep (n_keys around 64, 128, 512), 8 lanes
    per key; n_keys smaller than the sequence (trailing rows keep their prefill), q_row / kv_row0 / do_row non-zero; accumulate: ref = bf16 prefill + exact, bar
    + u |sum|.  dq is written on the query row only, columns beyond 3 * heads * 64 never."""
    q_row, kv_row0, do_row, extra = rows
    rc, c = _cls_bwd_case(gpu, n_keys, H, q_row=q_row, kv_row0=kv_row0, do_row=do_row, extra=extra, accumulate=accumulate, seed=n_keys)
    _ok(rc, 'sf_attention_cls_bwd')
    torch.cuda.synchronize()
    n, R, Hd, ldg = c['n'], c['R'], c['Hd'], c['ldg']
    x = c['qkv'].double().view(n, R, c['ld'])
    kv = slice(kv_row0, kv_row0 + n_keys)
    Q = x[:, q_row, :Hd].reshape(n, 1, H, 64).permute(0, 2, 1, 3).reshape(n * H, 1, 64)
    K = x[:, kv, Hd:2 * Hd].reshape(n, n_keys, H, 64).permute(0, 2, 1, 3).reshape(n * H, n_keys, 64)
    V = x[:, kv, 2 * Hd:3 * Hd].reshape(n, n_keys, H, 64).permute(0, 2, 1, 3).reshape(n * H, n_keys, 64)
    dO = c['dO'].double().view(n, c['Rdo'], c['lddo'])[:, do_row, :Hd].reshape(n * H, 1, 64)
    r = _core(Q, K, V, dO, 0.125, round_mid=False)
    raw = c['d'].cpu()
    got, pre = raw.double().view(n, R, ldg), c['pre'].double().view(n, R, ldg)
    name = 'sf_attention_cls_bwd'
    sec = _direct(r['dq'].reshape(n, H, 64), 0, r['F_dq'].reshape(n, H, 64), r['e_dq'].reshape(n, H, 64))
    _check_section(name, 'dq', got[:, q_row, :Hd].reshape(n, H, 64), sec)
    for i, x_ in ((1, 'dk'), (2, 'dv')):
        shp = lambda t: t.reshape(n, 1, H, n_keys, 64)                             # noqa: E731
        ref, F = shp(r[x_]), shp(r['F_' + x_])
        if accumulate:
            p0 = pre[:, kv, i * Hd:(i + 1) * Hd].reshape(n, n_keys, H, 64).permute(0, 2, 1, 3).reshape(n, 1, H, n_keys, 64)
            ref = ref + p0
            F = F + 2 * U32 * ref.abs()
        sec = _Sec(ref, MARGIN * (U * shp(r[x_]).abs() + F) + (U * ref.abs() if accumulate else 0), _rb(ref), F)
        g_ = got[:, kv, i * Hd:(i + 1) * Hd].reshape(n, n_keys, H, 64).permute(0, 2, 1, 3).reshape(n, 1, H, n_keys, 64)
        _check_section(name, x_, g_, sec)
    written = torch.zeros(n, R, ldg, dtype=torch.bool)
    written[:, q_row, :Hd] = True
    written[:, kv, Hd:3 * Hd] = True
    _assert_untouched(raw, c['pre'], written.view(n * R, ldg), name)


@pytest.mark.gpu
def test_cls_bwd_sharp(gpu):
    rc, c = _cls_bwd_case(gpu, 513, 2, mode='sharp', seed=1)
    _ok(rc, 'sf_attention_cls_bwd')
    torch.cuda.synchronize()
    n, R, H, Hd = c['n'], c['R'], c['H'], c['Hd']
    x = c['qkv'].double().view(n, R, c['ld'])
    hs = lambda t: t.reshape(n, -1, H, 64).permute(0, 2, 1, 3).reshape(n * H, -1, 64)   # noqa: E731
    r = _core(hs(x[:, :1, :Hd]), hs(x[:, :513, Hd:2 * Hd]), hs(x[:, :513, 2 * Hd:3 * Hd]), hs(c['dO'].double().view(n, c['Rdo'], c['lddo'])[:, :1, :Hd]), 0.125, False)
    got = c['d'].cpu().double().view(n, R, c['ldg'])
    for i, x_ in enumerate(('dq', 'dk', 'dv')):
        rows = slice(0, 1) if i == 0 else slice(0, 513)
        g_ = got[:, rows, i * Hd:(i + 1) * Hd].reshape(n, -1, H, 64).permute(0, 2, 1, 3).reshape(n, 1, H, -1, 64)
        shp = lambda t: t.reshape(n, 1, H, -1, 64)                                 # noqa: E731
        _check_section('sf_attention_cls_bwd', x_ + ' (sharp)', g_, _direct(shp(r[x_]), 0, shp(r['F_' + x_]), shp(r['e_' + x_])))


@pytest.mark.gpu
def test_cls_bwd_rejects_2049_keys(gpu):
    rc, c = _cls_bwd_case(gpu, 2049, 1, n=1)
    _rejected(rc, 'n_keys = 2049')
    torch.cuda.synchronize()
    assert torch.equal(c['d'].cpu().view(torch.int16), c['pre'].view(torch.int16))


# ======================================================================================================================================
# 5. sf_attention_cls_stats / sf_attention_cls_combine_stats: the statistics themselves
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('G,T,mode', [(1, 33, 'normal'), (8, 196, 'normal'), (8, 7, 'normal'), (1, 196, 'cls_key_dominant'), (8, 33, 'cls_key_dominant'), (8, 196, 'sharp')])
def test_cls_statistics_against_float64(gpu, G, T, mode):
    """(m, l) of both producers against float64 for 1 and 8 partial groups and for sharp softmaxes: m is the maximum in the base-2 domain (max_j s_j log2 e, within
    its fp32 rounding and the scores' dot error), and m + log2 l against log2 sum_j exp s_j with the fp32 bars of _check_lse2; the two producers agree within the
    sum of their bars."""
    c = _Case(gpu, n=2, G=G, H=3, T=T, cls=True, mode='cls_key_dominant' if mode != 'normal' else 'normal', seed=3)
    if mode == 'sharp':                                                            # the CLS query 6 x a token key of the last group instead
        x = c.qkv_h.float().view(c.n, c.R, c.ld)
        x[:, 0, :c.Hd] = 6 * x[:, c.R - 3, c.Hd:2 * c.Hd]
        c.qkv_h = x.view(-1, c.ld).to(BF)
        c.qkv = c.qkv_h.to(gpu)
    q, k, v, dO = c.wide()
    ref = grouped_attention_bwd_ref(q, k, v, dO, c.geo, 0.125, clsq=True)
    keys = k[:, :1 + G * T]
    both = []
    for via in ('combine', 'cls_stats'):
        att, stats = c.forward_stats(0.125, via)
        torch.cuda.synchronize()
        st = stats.cpu().double().view(c.n, c.H, 2)
        both.append(_check_lse2(f'sf_attention_cls_{"combine_" if via == "combine" else ""}stats', st, ref['lse2'], q[:, 0], keys, 0.125))
    assert ((both[0][0] - both[1][0]).abs() <= both[0][1] + both[1][1]).all(), 'the two producers of the statistics disagree'


# ======================================================================================================================================
# 6. sf_softmax_rows / sf_softmax_bwd_rows
# ======================================================================================================================================
def _lpads(L):
    return sorted({L, -(-L // 32) * 32, 256})


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 2, 63, 64, 65, 184, 198, 255, 256])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 37])
def test_softmax_rows(gpu, L, rows):
    """P = bf16(exp(s - m) / sum) from fp32: bar = 1 bf16 ulp of the reference + ref * e * (2 |s - m| + 2 |s| + L + 16) (__expf's argument, the scaled score, the
    L-term sum, the division) + 2^-126 (an exponential below the smallest normal fp32 number is flushed to zero by v_exp_f32).  Scaled scores reach +-80; rows
    sum to 1 within L u; P[:, L:L_pad] is exactly zero and nothing beyond L_pad or in other rows' padding is touched; lds != ldp; four rows per workgroup."""
    g = _gen(L * 100 + rows)
    lds_, ldp = 264, 272
    scale = 0.125 if rows % 2 else 1.0
    S = (torch.randn(rows, lds_, generator=g) * 12).clamp(-80, 80)
    if L > 1:
        S[0, 0], S[0, L - 1] = 80.0, -80.0
    S = S / scale                                                                  # the SCALED scores span +-80 (a power-of-two scale: exact)
    Sd = S.to(gpu)
    for L_pad in _lpads(L):
        can = _canary(rows, ldp, L_pad)
        P = can.clone().to(gpu)
        _ok(_lib().sf_softmax_rows(Sd.data_ptr(), lds_, P.data_ptr(), ldp, rows, L, L_pad, scale, _st()), 'sf_softmax_rows')
        torch.cuda.synchronize()
        raw = P.cpu()
        got = raw.double()
        s = (S[:, :L] * scale).double()                                           # the kernel's fp32 product S * scale (exact here), widened
        m = s.amax(-1, keepdim=True)
        ref = torch.softmax(s, -1)
        bar = _bf16_ulp(ref) + ref * U32 * (2 * (s - m).abs() + 2 * s.abs() + L + 16) + 2.0 ** -126
        assert torch.isfinite(got[:, :L]).all()
        err = (got[:, :L] - ref).abs()
        WORST['sf_softmax_rows'] = max(WORST.get('sf_softmax_rows', 0.0), (err / bar).max().item())
        assert (err <= bar).all(), f'L {L} L_pad {L_pad}: worst err / bar {(err / bar).max().item():.3g} at {(err / bar).argmax().item()}'
        assert ((got[:, :L].sum(-1) - 1).abs() <= L * U).all()
        assert (raw[:, L:L_pad].view(torch.int16) == 0).all(), 'padding must be +0'
        written = torch.zeros(rows, ldp, dtype=torch.bool)
        written[:, :L_pad] = True
        _assert_untouched(raw, can, written, 'sf_softmax_rows')


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 2, 63, 64, 65, 184, 198, 255, 256])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 37])
def test_softmax_bwd_rows(gpu, L, rows):
    """dS = bf16(scale p (dP - sum_j p_j dP_j)) from the bf16 P and fp32 dP: bar = 1 bf16 ulp of the reference + scale p ((L + 8) e sum_j |p_j dP_j| + 4 e (|dP| + |dot|))
    (the L-term dot seen through the cancellation, the two products)."""
    g = _gen(L * 100 + rows + 7)
    ldp, lddp, ldds = 272, 264, 280
    P = torch.zeros(rows, ldp)
    P[:, :L] = torch.softmax(torch.randn(rows, L, generator=g) * 3, -1)
    P[:, L:] = 5.0                                                                 # must not be read
    P = P.to(BF)
    dP = torch.randn(rows, lddp, generator=g) * 2
    Pd, dPd = P.to(gpu), dP.to(gpu)
    for L_pad in _lpads(L):
        can = _canary(rows, ldds, L_pad)
        dS = can.clone().to(gpu)
        _ok(_lib().sf_softmax_bwd_rows(Pd.data_ptr(), ldp, dPd.data_ptr(), lddp, dS.data_ptr(), ldds, rows, L, L_pad, 0.125, _st()), 'sf_softmax_bwd_rows')
        torch.cuda.synchronize()
        raw = dS.cpu()
        p, gd = P[:, :L].double(), dP[:, :L].double()
        dot = (p * gd).sum(-1, keepdim=True)
        ref = 0.125 * p * (gd - dot)
        bar = _bf16_ulp(ref) + 0.125 * p * ((L + 8) * U32 * (p * gd).abs().sum(-1, keepdim=True) + 4 * U32 * (gd.abs() + dot.abs()))
        err = (raw[:, :L].double() - ref).abs()
        WORST['sf_softmax_bwd_rows'] = max(WORST.get('sf_softmax_bwd_rows', 0.0), (err / bar).max().item())
        assert (err <= bar).all(), f'L {L} L_pad {L_pad}: worst err / bar {(err / bar).max().item():.3g}'
        assert (raw[:, L:L_pad].view(torch.int16) == 0).all(), 'padding must be +0'
        written = torch.zeros(rows, ldds, dtype=torch.bool)
        written[:, :L_pad] = True
        _assert_untouched(raw, can, written, 'sf_softmax_bwd_rows')


@pytest.mark.gpu
def test_softmax_rows_reject_257(gpu):
    S = torch.zeros(4, 264, device=gpu)
    P = torch.zeros(4, 272, device=gpu, dtype=BF)
    _rejected(_lib().sf_softmax_rows(S.data_ptr(), 264, P.data_ptr(), 272, 4, 257, 257, 1.0, _st()), 'L = 257')
    _rejected(_lib().sf_softmax_rows(S.data_ptr(), 264, P.data_ptr(), 272, 4, 200, 257, 1.0, _st()), 'L_pad = 257')
    _rejected(_lib().sf_softmax_bwd_rows(P.data_ptr(), 272, S.data_ptr(), 264, P.data_ptr(), 272, 4, 257, 257, 1.0, _st()), 'bwd L = 257')
    _rejected(_lib().sf_softmax_bwd_rows(P.data_ptr(), 272, S.data_ptr(), 264, P.data_ptr(), 272, 4, 200, 257, 1.0, _st()), 'bwd L_pad = 257')


# ======================================================================================================================================
# 7. sf_reduce_groups_bf16
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('G,cols,gstride_pad,seq_pad', [(8, 768, 0, 0), (9, 1536, 8, 16), (16, 8, 0, 8), (17, 520, 8, 0), (196, 1536, 0, 0), (196, 520, 16, 8),  # vector
                                                         (1, 5, 0, 0), (7, 770, 1, 3), (7, 5, 3, 1), (1, 770, 0, 1), (9, 770, 0, 0), (7, 768, 0, 0)])                # scalar
@pytest.mark.parametrize('n_seq', [1, 3])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_reduce_groups(gpu, G, cols, gstride_pad, seq_pad, n_seq, accumulate):
    """out (=|+=) sum_g in[g]: fp32 sum, one bf16 store.  bar = 1 bf16 ulp of the float64 sum + G e sum |terms| (G additions at most: G - 1 of the
    groups, one of the prefill, whose absolute value then counts among the terms).  Vector kernel (cols % 8 == 0, G >= 8, aligned
    strides; 16 group slices x 512 columns per workgroup: G = 9, 17, 196 leave ragged slices, cols = 520 a ragged workgroup) and scalar kernel (G < 8, odd columns or
    strides); the columns between `cols` and the strides keep their canary."""
    g = _gen(G * 1000 + cols + n_seq)
    gstr = cols + gstride_pad
    sstr = G * gstr + seq_pad
    ostr = cols + (8 if cols % 8 == 0 and gstride_pad % 8 == 0 and seq_pad % 8 == 0 else 3)
    src = (torch.randn(n_seq * sstr, generator=g) * 0.7).to(BF)
    can = _canary(n_seq, ostr, G)
    if accumulate:
        can = (torch.randn(n_seq, ostr, generator=g) * 0.5 + 1.5).to(BF)
    out, srcd = can.clone().to(gpu), src.to(gpu)
    _ok(_lib().sf_reduce_groups_bf16(srcd.data_ptr(), sstr, gstr, G, out.data_ptr(), ostr, cols, n_seq, accumulate, _st()), 'sf_reduce_groups_bf16')
    torch.cuda.synchronize()
    raw = out.cpu()
    terms = torch.stack([src[s * sstr:s * sstr + G * gstr].view(G, gstr)[:, :cols] for s in range(n_seq)]).double()     # (n_seq, G, cols)
    ref, sabs = terms.sum(1), terms.abs().sum(1)
    if accumulate:
        ref, sabs = ref + can[:, :cols].double(), sabs + can[:, :cols].double().abs()
    bar = _bf16_ulp(ref) + G * U32 * sabs
    err = (raw[:, :cols].double() - ref).abs()
    WORST['sf_reduce_groups_bf16'] = max(WORST.get('sf_reduce_groups_bf16', 0.0), (err / bar).max().item())
    assert (err <= bar).all(), f'worst err / bar {(err / bar).max().item():.3g} at column {int((err / bar).max(0).values.argmax())}'
    written = torch.zeros(n_seq, ostr, dtype=torch.bool)
    written[:, :cols] = True
    _assert_untouched(raw, can, written, 'sf_reduce_groups_bf16')


@pytest.mark.gpu
def test_zz_report_worst_ratios(gpu):
    """Prints the worst observed error / bar ratio per kernel of this run (pytest -s); asserts nothing beyond what the tests above did."""
    for name in sorted(WORST):
        print(f'worst ratio  {name}: {WORST[name]:.3f}')
