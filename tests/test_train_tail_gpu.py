"""GPU: the kernels that close a train step (csrc/sf_train.hip: sf_softmax_rows, sf_softmax_bwd_rows, sf_colsum, sf_cross_entropy, sf_adam_clip_step), the Stage-1
head (csrc/sf_clip.hip: sf_meanpool_l2norm768, sf_similarity_f32, sf_shift_window_preds) and the tower-backward helpers (csrc/sf_towerbwd.hip:
sf_meanpool_l2norm768_bwd, sf_reduce_groups_bf16) against float64 restatements computed on the host from the very bf16 / fp32 values each kernel reads.  References,
bars and verdicts are tests/train_tail_oracle.py's (each bar's derivation is in the docstring of its function there; tests/test_train_tail_oracle_cpu.py shows that
they reject a subtly wrong kernel).  Conventions, as in tests/test_train_rowops_gpu.py: bit for bit where the arithmetic is exact (integer operands, pad zeros, the
bf16 copy of Adam's p, C = 1 in the cross-entropy, an all-zero pooled group), bars relative to the sum of absolute terms elsewhere, position-dependent canaries on
every byte that must not be written (pad columns, rows behind the last one, the workspace beyond its documented size), accumulate flags both ways on a non-zero
prefill, strided operands as column slices of wider buffers whose other elements are NaN.  Every launch stays inside its header contract.

Chain depths d:  softmax forward and backward 4 + 6 (four terms per lane, wave_sum's six levels);  colsum: train_tail_oracle.colsum_depth (scalar first stage 64 | 256
rows in sequence, vector first stage 2 | 8 rows per lane + 3 shuffles + 2 LDS levels; second stage ceil(nblk / 64) + 3 + 2 + 16, + the accumulate add);  cross-entropy
ceil(C / 64) + 6 per row and B additions over rows;  mean-pool t for the mean and 12 + 6 for the sum of squares;  similarity d;  reduce_groups ceil(G / 16) + 15 (vector
kernel) | G (scalar kernel), + the accumulate add.
The hardware exponential behind __expf (softmax, cross-entropy) is not derivable from this code: the bars ASSUME the ISA's documented accuracy of v_exp_f32, 1 ulp
(2^-23 relative), plus the rounding of its argument, |x - m| 2^-23.

Measured on an MI355X (gfx950): 63 tests, 4.9 s (slowest: colsum at 16383 rows, 0.4 s); no bug found.  Worst error / bar per kernel:  softmax forward 0.999, backward
1.000 and reduce_groups 1.000 (a bf16 output sits up to exactly half an ulp from the reference: the rounding itself fills the bar, the fp32 term is a few 1e-5 of it);
colsum 0.035;  cross-entropy loss 0.20, gradient 0.80 (the +-80 spread);  Adam m 0.42, v 0.28, p 0.998 (the half-ulp of the final subtraction);  mean-pool forward 0.25,
backward 0.44;  similarity 0.25 (d = 16), 0.006 (d = 768);  the exact similarity cases, the pad zeros, C = 1, the zero group, p_bf16 and every prediction bit for bit.
The v_exp_f32 assumption held with that margin: no softmax or cross-entropy element came closer to its bar than the bf16 rounding / 0.80."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402
import train_tail_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _lib():
    from synchformer_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from synchformer_amd import _lib as L
    L.check(rc, what)


def _strided(values, ld):
    """`values` (rows, cols) as the leading columns of a (rows, ld) buffer that holds NaN elsewhere."""
    rows, cols = values.shape
    buf = torch.full((rows, ld), NAN, dtype=values.dtype)
    buf[:, :cols] = values
    return buf


def _report(name, stats):
    print(f'[{name}] ' + ', '.join(f'{k} {v:.3g}' for k, v in sorted(stats.items())))


# ======================================================================================================================================
# sf_softmax_rows / sf_softmax_bwd_rows
# ======================================================================================================================================
@pytest.mark.parametrize('L', T.SOFTMAX_L)
def test_softmax_rows_fwd_bwd_vs_fp64(gpu, L):
    """L_pad in {L, L rounded up to 32, 256}, rows in {1, 5, 8}, scale in {0.125, 1}, logits flat / sharp / spread down to -80 / the same plus 10^4; S, P, dP and dS
    all strided with NaN / canaries beyond their width.  Forward: |got - ref| <= bf16_ulp(ref) / 2 + F (train_tail_oracle.softmax_reference), P[L:L_pad] = 0 exactly.
    Backward from the bf16 P of the forward launch and an fp32 dP built from it (train_tail_oracle.softmax_bwd_dp; by row: Gaussian - the only row when rows = 1 -,
    constant, so that dP - sum p dP cancels to P's rounding, and dP_j = +-1 / p_j in pairs, so that sum p dP itself cancels to below 1e-6 sum |p dP|):
    |got - ref| <= bf16_ulp(ref) / 2 + MARGIN (d + 3) 2^-24 scale p (|dP| + sum |p dP|)."""
    lib, stats = _lib(), {}
    for rows in T.SOFTMAX_ROWS:
        for kind in T.SOFTMAX_KINDS:
            for scale in T.SOFTMAX_SCALES:
                S = T.softmax_logits(kind, rows, L, scale, seed=L + rows)
                lds, lddp = L + 3, L + 1
                Sd = _strided(S, lds).to(gpu)
                for L_pad in T.softmax_lpads(L):
                    ldp, ldds = L_pad + 5, L_pad + 7
                    preP, preD = G.canary((rows + 1, ldp), torch.bfloat16), G.canary((rows + 1, ldds), torch.bfloat16)
                    Pd, dSd = preP.to(gpu), preD.to(gpu)
                    _ok(lib.sf_softmax_rows(Sd.data_ptr(), lds, Pd.data_ptr(), ldp, rows, L, L_pad, scale, _st()), 'sf_softmax_rows')
                    P = Pd.cpu()
                    dP = T.softmax_bwd_dp(P[:rows, :L], seed=L * 7 + rows)       # from the P the backward will read: row 2's dot product cancels against it
                    dPd = _strided(dP, lddp).to(gpu)
                    _ok(lib.sf_softmax_bwd_rows(Pd.data_ptr(), ldp, dPd.data_ptr(), lddp, dSd.data_ptr(), ldds, rows, L, L_pad, scale, _st()), 'sf_softmax_bwd_rows')
                    dS = dSd.cpu()
                    what = f'rows {rows} {kind} scale {scale} L_pad {L_pad}'
                    msgs = T.softmax_verdict(S, scale, L_pad, P[:rows], preP[:rows], stats) + T.damage(P[rows:], preP[rows:], torch.zeros(1, ldp, dtype=torch.bool), 'P row behind')
                    msgs += T.softmax_bwd_verdict(P[:rows, :L], dP, scale, L_pad, dS[:rows], preD[:rows], stats)
                    msgs += T.damage(dS[rows:], preD[rows:], torch.zeros(1, ldds, dtype=torch.bool), 'dS row behind')
                    assert not msgs, what + ': ' + '\n'.join(msgs)
    _report(f'softmax L={L}', stats)


# ======================================================================================================================================
# sf_colsum
# ======================================================================================================================================
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('rows', T.COLSUM_ROWS)
def test_colsum_vs_fp64(gpu, rows, bf16):
    """rows across the rows_per_blk switch (64 below 16384 rows, 256 from there), cols in {21, 32, 64, 96, 768} (96: the vector path for fp32, the scalar path for bf16),
    a base pointer offset by one element (the scalar path at a vector shape), accumulate both ways on a non-zero prefill; x is a slice of a NaN buffer with ld > cols,
    the workspace has its documented size cols * ceil(rows / 64) with a canary behind it.  |got - ref| <= (d + 1) 2^-24 (sum |x| + |prefill|), d from the path's tree."""
    lib, stats = _lib(), {}
    dt = torch.bfloat16 if bf16 else torch.float32
    for cols in T.COLSUM_COLS:
        x = (torch.randn(rows, cols, generator=G.gen(rows + cols)) * 2.0 + 0.25).to(dt)
        ld = cols + 8
        for off in ((0, 1) if T.colsum_is_vec(cols, bf16, True) else (0,)):
            flat = torch.full((rows * ld + 16,), NAN, dtype=dt)
            torch.as_strided(flat, (rows, cols), (ld, 1), off).copy_(x)
            flat = flat.to(gpu)
            xv = torch.as_strided(flat, (rows, cols), (ld, 1), off)
            assert (xv.data_ptr() % 16 == 0) == (off == 0)
            vec = T.colsum_is_vec(cols, bf16, off == 0)
            n_ws = T.colsum_workspace(rows, cols)
            pre = torch.randn(cols, generator=G.gen(cols))
            for acc in (False, True):
                pre_ws, pre_out = G.canary((n_ws + 64,), torch.float32), G.canary((cols + 16,), torch.float32)
                if acc:
                    pre_out[:cols] = pre
                ws, out = pre_ws.to(gpu), pre_out.to(gpu)
                _ok(lib.sf_colsum(xv.data_ptr(), int(bf16), ld, rows, cols, out.data_ptr(), int(acc), ws.data_ptr(), _st()), 'sf_colsum')
                o, w = out.cpu(), ws.cpu()
                msgs = T.colsum_verdict(x, pre, acc, vec, o[:cols], stats)
                msgs += T.damage(o[cols:], pre_out[cols:], torch.zeros(16, dtype=torch.bool), 'behind out') + T.damage(w[n_ws:], pre_ws[n_ws:], torch.zeros(64, dtype=torch.bool), 'behind the workspace')
                assert not msgs, f'cols {cols} offset {off} accumulate {acc} ({"vector" if vec else "scalar"} path): ' + '\n'.join(msgs)
    _report(f'colsum rows={rows} {"bf16" if bf16 else "f32"}', stats)


# ======================================================================================================================================
# sf_cross_entropy
# ======================================================================================================================================
@pytest.mark.parametrize('kind', T.CE_KINDS)
def test_cross_entropy_vs_fp64(gpu, kind):
    """B in {1, 16, 33}, C in {1, 2, 21, 64, 65, 130}, Gaussian / +-80 spread / +10^4 offset logits, ld > C and ldd > C (NaN / canaries beyond C), dlogits NULL and
    present (the loss must be bit-identical), grad_scale in {1, 0.25}.  Loss bar relative to mean(|m| + |log s| + |z_t|), gradient elementwise (train_tail_oracle.ce_reference);
    C = 1: loss and gradient exactly 0."""
    lib, stats = _lib(), {}
    for B in T.CE_B:
        for C in T.CE_C:
            z, tgt = T.ce_logits(kind, B, C, seed=B * 131 + C)
            ld, ldd = C + 3, C + 5
            zd, td = _strided(z, ld).to(gpu), tgt.to(gpu)
            for gs in (1.0, 0.25):
                pre = G.canary((B + 1, ldd), torch.float32)
                dz, loss, loss0 = pre.to(gpu), torch.full((4,), NAN, device=gpu), torch.full((4,), NAN, device=gpu)
                _ok(lib.sf_cross_entropy(zd.data_ptr(), ld, td.data_ptr(), B, C, loss.data_ptr(), dz.data_ptr(), ldd, gs, _st()), 'sf_cross_entropy')
                _ok(lib.sf_cross_entropy(zd.data_ptr(), ld, td.data_ptr(), B, C, loss0.data_ptr(), None, 0, gs, _st()), 'sf_cross_entropy')
                d, l, l0 = dz.cpu(), loss.cpu(), loss0.cpu()
                msgs = T.ce_verdict(z, tgt, gs, l[0], d[:B, :C], stats) + T.same_bits(l0[:1], l[:1], 'loss without dlogits')
                written = torch.zeros(B + 1, ldd, dtype=torch.bool)
                written[:B, :C] = True
                msgs += T.damage(d, pre, written, 'dlogits')
                assert torch.isnan(l[1:]).all() and torch.isnan(l0[1:]).all(), 'written behind the loss'
                assert not msgs, f'B {B} C {C} grad_scale {gs}: ' + '\n'.join(msgs)
    _report(f'cross_entropy {kind}', stats)


# ======================================================================================================================================
# sf_adam_clip_step
# ======================================================================================================================================
def _adam_launch(lib, gpu, p, g, m, v, norm, max_norm, step, with_bf16):
    n, hp = p.numel(), T.ADAM_HP
    pad = lambda t: torch.cat([t, G.canary((16,), torch.float32)]).to(gpu)
    pd, md, vd = pad(p), pad(m), pad(v)
    gd = torch.cat([g, torch.full((16,), NAN)]).to(gpu)
    pre_b = G.canary((n + 16,), torch.bfloat16)
    pb = pre_b.to(gpu)
    nd = torch.tensor([float(norm), NAN], device=gpu) if norm is not None else None
    _ok(lib.sf_adam_clip_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), pb.data_ptr() if with_bf16 else None, n, nd.data_ptr() if nd is not None else None,
                              max_norm, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step, _st()), 'sf_adam_clip_step')
    pn, mn, vn, pbn = pd.cpu(), md.cpu(), vd.cpu(), pb.cpu()
    tail = G.canary((16,), torch.float32)
    for name, t in (('p', pn), ('m', mn), ('v', vn)):
        assert torch.equal(G.bits(t[n:]), G.bits(tail)), f'written behind {name}'
    assert torch.equal(G.bits(pbn[n if with_bf16 else 0:]), G.bits(pre_b[n if with_bf16 else 0:])), 'written behind p_bf16 (or into it without being asked)'
    return pn[:n], mn[:n], vn[:n], (pbn[:n] if with_bf16 else None)


@pytest.mark.parametrize('n', T.ADAM_N)
def test_adam_clip_step_vs_fp64(gpu, n):
    """n around the 256-thread block and 100003; p_bf16 present and NULL; max_norm <= 0 with norm = NULL, the clip inactive, active, and with the norm in the buffer one
    ulp below / at / one ulp above max_norm; step in {1, 2, 1000, 100000}; three consecutive steps carrying m and v.  The float64 reference uses the fp32-rounded lr,
    beta1, beta2, eps and 1 - beta^step of those; m and v within 6 | 10 roundings of their two terms, p within 2^-24 |p| + (6 2^-24 + the launcher's bias-correction
    error) |dp|, p_bf16 bit for bit the RNE rounding of the returned p, nothing written beyond n."""
    lib, stats = _lib(), {}
    gen = G.gen(n)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3
    m, v = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01 + 1e-7
    gn = g.double().norm().float()                                   # ||g|| as an fp32 value: what the buffer holds
    one = torch.tensor(1.0)
    clips = [(None, 0.0), (None, -1.0), (gn, float(gn) * 4), (gn, float(gn) * 0.37), (torch.nextafter(gn, 0 * one), float(gn)), (gn, float(gn)),
             (torch.nextafter(gn, 1e9 * one), float(gn))]
    for step in T.ADAM_STEPS:
        for norm, max_norm in clips:
            for with_bf16 in (True, False):
                pn, mn, vn, pbn = _adam_launch(lib, gpu, p, g, m, v, norm, max_norm, step, with_bf16)
                msgs = T.adam_verdict(p, g, m, v, norm, max_norm, step, pn, mn, vn, pbn, stats)
                assert not msgs, f'step {step} norm {norm} max_norm {max_norm} bf16 {with_bf16}: ' + '\n'.join(msgs)
    for with_bf16 in (True, False):                                  # three consecutive steps: each one checked from the state the previous one returned
        pc, mc, vc = p, m, v
        for step in (1, 2, 3):
            gs = torch.randn(n, generator=gen) * 0.3
            pn, mn, vn, pbn = _adam_launch(lib, gpu, pc, gs, mc, vc, gn, float(gn) * 0.5, step, with_bf16)
            msgs = T.adam_verdict(pc, gs, mc, vc, gn, float(gn) * 0.5, step, pn, mn, vn, pbn, stats)
            assert not msgs, f'consecutive step {step}: ' + '\n'.join(msgs)
            pc, mc, vc = pn, mn, vn
    _report(f'adam n={n}', stats)


# ======================================================================================================================================
# sf_meanpool_l2norm768 and its backward
# ======================================================================================================================================
@pytest.mark.parametrize('t', T.POOL_T)
@pytest.mark.parametrize('n', T.POOL_N)
def test_meanpool_l2norm768_fwd_bwd_vs_fp64(gpu, n, t):
    """normalize 0 and 1, ldx / ldy / lddy / lddx > 768 with NaN / canaries beyond 768 columns and behind the last row.  Forward at three magnitudes (pooled-row norms
    about 1e-13, 30 and 1e14: inside [1e-15, 1e15], see train_tail_oracle.meanpool_reference) and with an all-zero group, whose output row must be exactly zero through the
    1e-12 clamp.  Backward with the derived bar of train_tail_oracle.meanpool_bwd_reference."""
    lib, stats = _lib(), {}
    gen = G.gen(n * 10 + t)
    ldx, ldy, lddy, lddx = 768 + 4, 768 + 8, 768 + 12, 768 + 16
    for mag in (3e-15, 1.0, 3e12):
        x = torch.randn(n * t, 768, generator=gen) * mag
        x[(n - 1) * t:] = 0.0 if mag == 1.0 else x[(n - 1) * t:]      # the last group all zero
        xd = _strided(x, ldx).to(gpu)
        for normalize in (0, 1):
            pre = G.canary((n + 1, ldy), torch.float32)
            yd = pre.to(gpu)
            _ok(lib.sf_meanpool_l2norm768(xd.data_ptr(), ldx, t, yd.data_ptr(), ldy, normalize, n, _st()), 'sf_meanpool_l2norm768')
            y = yd.cpu()
            ref, bar = T.meanpool_reference(x, t, normalize)
            msgs = T.within(y[:n, :768], ref, bar, 'meanpool', stats, 'meanpool fwd')
            written = torch.zeros(n + 1, ldy, dtype=torch.bool)
            written[:n, :768] = True
            msgs += T.damage(y, pre, written, 'y')
            if mag == 1.0:
                msgs += T.same_bits(y[n - 1, :768], torch.zeros(768), 'the all-zero group')
            assert not msgs, f'magnitude {mag} normalize {normalize}: ' + '\n'.join(msgs)
    x = torch.randn(n * t, 768, generator=gen) * 0.7 + 0.1
    dy = torch.randn(n, 768, generator=gen)
    xd, dyd = _strided(x, ldx).to(gpu), _strided(dy, lddy).to(gpu)
    for normalize in (0, 1):
        pre = G.canary((n * t + 1, lddx), torch.float32)
        dxd = pre.to(gpu)
        _ok(lib.sf_meanpool_l2norm768_bwd(xd.data_ptr(), ldx, t, dyd.data_ptr(), lddy, dxd.data_ptr(), lddx, normalize, n, _st()), 'sf_meanpool_l2norm768_bwd')
        dx = dxd.cpu()
        ref, bar = T.meanpool_bwd_reference(x, dy, t, normalize)
        written = torch.zeros(n * t + 1, lddx, dtype=torch.bool)
        written[:n * t, :768] = True
        msgs = T.within(dx[:n * t, :768], ref, bar, 'meanpool backward', stats, 'meanpool bwd') + T.damage(dx, pre, written, 'dx')
        assert not msgs, f'backward normalize {normalize}: ' + '\n'.join(msgs)
    _report(f'meanpool n={n} t={t}', stats)


# ======================================================================================================================================
# sf_similarity_f32
# ======================================================================================================================================
@pytest.mark.parametrize('family', ['exact', 'wide'])
@pytest.mark.parametrize('d', T.SIM_D)
def test_similarity_f32_vs_fp64(gpu, d, family):
    """n, m in {1, 63, 64, 65, 130} (ragged 64 x 64 tiles in both directions, more than one tile), lda, ldb > d, ldo > m with canaries beyond m and behind row n - 1,
    scale in {1, 1000}.  Integer-valued operands: bit for bit (the integer sum is exact, the scale's product rounds once); Gaussian: (d + 1) 2^-24 scale sum |a b|."""
    lib, stats = _lib(), {}
    for n in T.SIM_SIZES:
        for m in T.SIM_SIZES:
            a, b = T.sim_operands(family, n, m, d, seed=n * 131 + m)
            lda, ldb, ldo = d + 4, d + 8, m + 3
            ad, bd = _strided(a, lda).to(gpu), _strided(b, ldb).to(gpu)
            for scale in T.SIM_SCALES:
                pre = G.canary((n + 1, ldo), torch.float32)
                od = pre.to(gpu)
                _ok(lib.sf_similarity_f32(ad.data_ptr(), lda, bd.data_ptr(), ldb, od.data_ptr(), ldo, n, m, d, scale, _st()), 'sf_similarity_f32')
                msgs = T.sim_verdict(family, a, b, scale, od.cpu(), pre, stats)
                assert not msgs, f'n {n} m {m} scale {scale}: ' + '\n'.join(msgs)
    _report(f'similarity d={d} {family}', stats)


# ======================================================================================================================================
# sf_shift_window_preds
# ======================================================================================================================================
@pytest.mark.parametrize('n_clips', [1, 3])
@pytest.mark.parametrize('S,W', T.SHIFT_CASES)
def test_shift_window_preds_vs_loops(gpu, S, W, n_clips):
    """Every clip's block a random integer matrix in [-8, 8] of its own (every window sum exact in fp32: no case needs skipping; the expected predictions differ
    between the clips and between the two directions, and change with W - tests/test_train_tail_oracle_cpu.py asserts it for every case) with ties planted into it - the
    first maximum must win along row 0 and along column n - 1 -, ldg > n_clips * S, everything outside the clips' diagonal blocks 1e30 (read once, it decides an
    argmax); against the explicit-loop float64 reference."""
    ldg, n = n_clips * S + 4, S - W + 1
    Gm = T.shift_operands(n_clips, S, W, ldg, seed=T.shift_seed(S, W))
    Gd = Gm.to(gpu)
    pa = torch.full((n_clips * n + 4,), -7, dtype=torch.int64, device=gpu)
    pv = pa.clone()
    _ok(_lib().sf_shift_window_preds(Gd.data_ptr(), ldg, n_clips, S, W, pa.data_ptr(), pv.data_ptr(), _st()), 'sf_shift_window_preds')
    pa, pv = pa.cpu(), pv.cpu()
    assert (pa[n_clips * n:] == -7).all() and (pv[n_clips * n:] == -7).all(), 'written behind the predictions'
    msgs = T.shift_verdict(Gm, n_clips, S, W, pa[:n_clips * n].view(n_clips, n), pv[:n_clips * n].view(n_clips, n))
    assert not msgs, '\n'.join(msgs)


# ======================================================================================================================================
# sf_reduce_groups_bf16
# ======================================================================================================================================
@pytest.mark.parametrize('Gn', T.RG_G)
def test_reduce_groups_bf16_vs_fp64(gpu, Gn):
    """cols in {8, 64, 520} and 60, n_seq in {1, 3}, accumulate both ways on a non-zero prefill; the vector path (cols % 8 == 0, G >= 8, strides % 8 == 0) and the
    scalar path (G < 8, cols = 60, or odd strides at a vector shape); group stride > cols with NaN between the groups, canaries between and behind the rows of out.
    |got - ref| <= bf16_ulp(ref) / 2 + (d + 1) 2^-24 (sum |x| + |prefill|)."""
    lib, stats = _lib(), {}
    gen = G.gen(Gn)
    for cols in T.RG_COLS + [60]:
        for n_seq in T.RG_NSEQ:
            x = torch.randn(n_seq, Gn, cols, generator=gen).bfloat16()
            prefill = torch.randn(n_seq, cols, generator=gen).bfloat16()
            for odd in (False, True):
                gs, oss = (cols + 3, cols + 1) if odd else (cols + 8, cols + 8)
                gs, oss = (gs + 4, oss + 4) if (not odd and cols == 60) else (gs, oss)      # cols = 60: 72 / 72, multiples of 8 - the ragged cols alone force the scalar path
                iss = Gn * gs + (5 if odd else 16)
                vec = T.reduce_groups_is_vec(Gn, cols, not odd)
                inb = torch.full((n_seq, iss), NAN, dtype=torch.bfloat16)
                torch.as_strided(inb, (n_seq, Gn, cols), (iss, gs, 1)).copy_(x)
                ind = inb.to(gpu)
                for acc in (False, True):
                    pre = G.canary((n_seq + 1, oss), torch.bfloat16)
                    if acc:
                        pre[:n_seq, :cols] = prefill
                    od = pre.to(gpu)
                    _ok(lib.sf_reduce_groups_bf16(ind.data_ptr(), iss, gs, Gn, od.data_ptr(), oss, cols, n_seq, int(acc), _st()), 'sf_reduce_groups_bf16')
                    o = od.cpu()
                    written = torch.zeros(n_seq + 1, oss, dtype=torch.bool)
                    written[:n_seq, :cols] = True
                    msgs = T.reduce_groups_verdict(x, prefill, acc, vec, o[:n_seq, :cols], stats) + T.damage(o, pre, written, 'out')
                    assert not msgs, f'cols {cols} n_seq {n_seq} odd strides {odd} accumulate {acc} ({"vector" if vec else "scalar"} path): ' + '\n'.join(msgs)
    _report(f'reduce_groups G={Gn}', stats)
