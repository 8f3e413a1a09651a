"""CPU: the harness of tests/test_wgrad_gemm_gpu.py and tests/test_train_tail_gpu.py would reject a subtly wrong kernel.  The fp32 emulations of
tests/train_tail_oracle.py stand in for a kernel's output: each one must pass its verdict as it is, and each of these corruptions - a
dropped or doubled token row, row M read, a row in the wrong chunk, swapped 16-byte chunks, a bias partial from the wrong tile, an unwritten empty chunk, softmax
without its max / over L_pad / rounded toward zero, a dropped colsum block, a cross-entropy gradient not divided by B, Adam with swapped bias corrections or a late
clip, a mean over t + 1, a similarity row written past n, an argmax that takes the last maximum / swaps its two outputs / sums W - 1 terms / reads the next
clip, a missing group - must fail it.  The float64 references are checked against explicit Python loops at tiny sizes, and the exactness bound (every partial sum below 2^24) is asserted for every integer case of the GPU grid.
81 tests, 5 s on the host; every corruption is rejected, every emulation accepted (as is every kernel on an MI355X: the figures are in the two GPU files)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402
import train_tail_oracle as T  # noqa: E402

TN_GRID = [('splitk',) + c for c in T.TN_SPLITK_CASES] + [('pp',) + c for c in T.TN_PP_CASES]
TN_IDS = [f'{c[0]}-{c[1]}-M{c[2]}-{c[3]}x{c[4]}-s{c[5]}-kc{c[6]}' for c in TN_GRID]


def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * max(1.0, abs(a), abs(b))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references against explicit loops
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_tn_reference_against_loops():
    M, N, K, split, kc = 70, 128, 128, 3, 64                     # 64 | 6 | 0 rows
    dy, x = T.tn_operands('wide', M, N, K, seed=3)
    assert torch.isnan(dy[M:].float()).all() and torch.isnan(x[M:].float()).all() and not torch.isnan(dy[:M].float()).any()
    part, S, bias, Sb = T.tn_reference(dy, x, M, split, kc)
    dl, xl = dy.double().tolist(), x.double().tolist()
    for s, i, j in ((0, 0, 0), (0, 127, 5), (1, 3, 127), (2, 9, 9)):
        rows = range(s * kc, min(M, (s + 1) * kc))
        assert _close(float(part[s, i, j]), sum(dl[m][i] * xl[m][j] for m in rows))
        assert _close(float(S[s, i, j]), sum(abs(dl[m][i] * xl[m][j]) for m in rows))
        assert _close(float(bias[s, i]), sum(dl[m][i] for m in rows)) and _close(float(Sb[s, i]), sum(abs(dl[m][i]) for m in rows))
    assert float(part[2].abs().max()) == 0.0 and float(bias[2].abs().max()) == 0.0


def test_marker_operands():
    M, N, K = 261, 128, 384
    dy, x = T.tn_operands('marker', M, N, K, seed=0)
    d = dy[:M].float()
    assert float(d.sum()) == M and all(float(d[m, m % N]) == 1.0 for m in range(M))
    assert x[:M].float().equal(x[:M].double().float()) and float(x[257, 0]) == 257 % 251 + 1 and float(x[257, 1]) == 2.0


def test_row_references_against_loops():
    g = G.gen(1)
    # softmax forward / backward
    S = torch.randn(2, 5, generator=g) * 3
    p, F = T.softmax_reference(S, 0.125)
    for r in range(2):
        xs = [float(S[r, c]) * 0.125 for c in range(5)]
        e = [math.exp(v - max(xs)) for v in xs]
        assert all(_close(float(p[r, c]), e[c] / sum(e)) for c in range(5))
    assert float(F.max()) < 1e-5
    P, dP = p.bfloat16(), torch.randn(2, 5, generator=g)
    ref, _ = T.softmax_bwd_reference(P, dP, 0.125)
    for r in range(2):
        dot = sum(float(P[r, c]) * float(dP[r, c]) for c in range(5))
        assert all(_close(float(ref[r, c]), 0.125 * float(P[r, c]) * (float(dP[r, c]) - dot)) for c in range(5))
    # cross-entropy
    z, tgt = T.ce_logits('gauss', 3, 4, seed=2)
    loss, _, grad, _ = T.ce_reference(z, tgt, 0.25)
    tot = 0.0
    for b in range(3):
        zs = [float(z[b, c]) for c in range(4)]
        lse = math.log(sum(math.exp(v - max(zs)) for v in zs)) + max(zs)
        tot += lse - zs[int(tgt[b])]
        for c in range(4):
            assert _close(float(grad[b, c]), (math.exp(zs[c] - lse) - (1.0 if c == int(tgt[b]) else 0.0)) * 0.25 / 3, 1e-10)
    assert _close(float(loss), tot / 3)
    # Adam, from the fp32-rounded hyper-parameters
    pp, gg, mm, vv = (torch.randn(3, generator=g) for _ in range(4))
    vv = vv.abs()
    r = T.adam_reference(pp, gg, mm, vv, torch.tensor(4.0), 1.0, 2)
    b1, b2, lr, eps = (float(torch.tensor(T.ADAM_HP[k], dtype=torch.float32)) for k in ('beta1', 'beta2', 'lr', 'eps'))
    coef = 1.0 / (4.0 + float(torch.tensor(1e-6, dtype=torch.float32)))
    for i in range(3):
        gi = float(gg[i]) * coef
        m1, v1 = b1 * float(mm[i]) + (1 - b1) * gi, b2 * float(vv[i]) + (1 - b2) * gi * gi
        assert _close(float(r['m'][i]), m1) and _close(float(r['v'][i]), v1)
    assert _close(r['bc1'], 1 - b1 * b1) and _close(r['bc2'], 1 - b2 * b2) and b2 != 0.999
    pref, _ = T.adam_p_reference(pp, mm, vv, r)
    assert _close(float(pref[0]), float(pp[0]) - lr * (float(mm[0]) / r['bc1']) / (math.sqrt(float(vv[0]) / r['bc2']) + eps))


def test_head_references_against_loops():
    g = G.gen(5)
    x = torch.randn(2 * 3, 768, generator=g)
    y, _ = T.meanpool_reference(x, 3, True)
    m0 = [sum(float(x[j, c]) for j in range(3)) / 3 for c in range(768)]
    nrm = math.sqrt(sum(v * v for v in m0))
    assert all(_close(float(y[0, c]), m0[c] / nrm) for c in (0, 5, 767))
    dy = torch.randn(2, 768, generator=g)
    dx, _ = T.meanpool_bwd_reference(x, dy, 3, True)
    dot = sum(m0[c] * float(dy[0, c]) for c in range(768))
    for c in (0, 767):
        want = (float(dy[0, c]) / nrm - m0[c] * dot / nrm ** 3) / 3
        assert _close(float(dx[0, c]), want) and _close(float(dx[2, c]), want)
    z, _ = T.meanpool_reference(torch.zeros(3, 768), 3, True)
    assert float(z.abs().max()) == 0.0
    # shift_and_get_preds on the similarity matrix, through the feature-space definition (a, v -> windows of W segments flattened -> argmax)
    S, W, Dm = 5, 3, 4
    a, v = torch.randint(-2, 3, (1, S, Dm), generator=g).double(), torch.randint(-2, 3, (1, S, Dm), generator=g).double()
    af, vf = a.unfold(-2, W, 1).reshape(1, S - W + 1, -1), v.unfold(-2, W, 1).reshape(1, S - W + 1, -1)
    sim = af @ vf.mT
    pa, pv = T.shift_reference((a[0] @ v[0].t()).float(), 1, S, W)
    assert pa.equal(torch.argmax(sim, -2)) and pv.equal(torch.argmax(sim, -1))
    # reduce_groups / colsum / similarity are plain sums: explicit loops pass the verdict, the same loops short of one term do not
    xg = torch.randn(2, 7, 8, generator=g).bfloat16()
    loop = lambda G_: torch.tensor([[sum(float(xg[s, k, c]) for k in range(G_)) for c in range(8)] for s in range(2)])
    assert T.reduce_groups_verdict(xg, torch.zeros(2, 8).bfloat16(), False, False, loop(7).bfloat16()) == []
    assert T.reduce_groups_verdict(xg, torch.zeros(2, 8).bfloat16(), False, False, loop(6).bfloat16())
    xc = torch.randn(5, 3, generator=g)
    loop = lambda R: torch.tensor([sum(float(xc[r, c]) for r in range(R)) for c in range(3)])
    assert T.colsum_verdict(xc, torch.zeros(3), False, False, loop(5)) == [] and T.colsum_verdict(xc, torch.zeros(3), False, False, loop(4))
    a, b = T.sim_operands('wide', 2, 3, 16, seed=1)
    loop = lambda D_: torch.tensor([[1000.0 * sum(float(a[i, k]) * float(b[j, k]) for k in range(D_)) for j in range(3)] for i in range(2)])
    pre = G.canary((2, 3), torch.float32)
    assert T.sim_verdict('wide', a, b, 1000.0, loop(16), pre) == [] and T.sim_verdict('wide', a, b, 1000.0, loop(15), pre)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the weight-gradient grid: exactness bounds, the emulation under both criteria, the corruptions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_grid_reaches_every_mechanism():
    nks, mods = set(), set()
    for fam, M, N, K, split, kc in T.TN_SPLITK_CASES:
        assert M < 700 and kc % 64 == 0 and split * kc >= M and N % 128 == 0 and K % 128 == 0
        ch = [hi - lo for lo, hi in T.tn_chunks(M, split, kc)]
        nks |= {-(-v // 32) for v in ch}
        mods.add([v for v in ch if v][-1] % 32)
    assert {0, 1, 2, 3, 4, 5, 9} <= nks and {1, 3, 5, 31} <= mods
    assert {(c[2], c[3]) for c in T.TN_SPLITK_CASES} >= {(128, 128), (128, 384), (384, 128), (384, 384), (256, 768)}
    items, lasts = set(), set()
    for fam, M, N, K, split, kc in T.TN_PP_CASES:
        assert kc % 128 == 0 and split * kc >= M > (split - 1) * kc and N % 256 == 0 and K % 256 == 0
        items.add(split * (N // 256) * (K // 256))
        last = M - (split - 1) * kc
        lasts.add('kc-1' if last == kc - 1 else last)
    assert {1, 7, 9, 11} <= items and {1, 63, 65, 'kc-1'} <= lasts and {c[5] for c in T.TN_PP_CASES} == {128, 256, 384}
    assert {(c[2], c[3]) for c in T.TN_PP_CASES} >= {(256, 256), (512, 256), (256, 512), (512, 768)}
    for blocks in (64, 256, 304):
        one, two = T.tn_pp_walk_cases(blocks)
        assert blocks < one[4] <= 2 * blocks < two[4] <= 3 * blocks
    assert T.tn_pp_walk_cases(256)[1][4] * 256 * 256 * 4 < 150e6      # part of the three-item walk on 256 workgroups: about 140 MB


@pytest.mark.parametrize('kernel,family,M,N,K,split,kc', TN_GRID, ids=TN_IDS)
def test_tn_case_exactness_and_emulation(kernel, family, M, N, K, split, kc):
    """Integer families: every partial sum stays below 2^24 (so the fp32 result cannot depend on chunking, ring order or swizzle) and the emulation reproduces the
    int64 result bit for bit.  wide: the emulation itself passes the elementwise and the statistical criterion."""
    dy, x = T.tn_operands(family, M, N, K, seed=M + N)
    if family != 'wide':
        assert T.tn_exact_bound(dy, x, M, kc) < 2 ** 24
    part, bias = T.tn_emulate(kernel, dy, x, M, split, kc)
    assert T.tn_verdict(kernel, family, dy, x, M, split, kc, part, bias) == []


def test_tn_walk_cases_exactness():
    for blocks in (8, 256, 304):
        for family, M, N, K, split, kc in T.tn_pp_walk_cases(blocks):
            assert family == 'exact' and kc * 4 * 8 < 2 ** 24 and (split - 1) * kc < M <= split * kc and split * kc * (N + 64) * 2 < 2 ** 32


def _first(cases, pred):
    return next(c for c in cases if pred(*c))


# sf_gemm_tn_pp refuses an empty chunk (asserted on the device), so no launch of it can leave one unwritten
TN_MUTATION_GRID = [(k, f, m) for k in ('splitk', 'pp') for f in ('exact', 'wide') for m in T.TN_MUTATIONS if not (k == 'pp' and m == 'empty_unwritten')]


@pytest.mark.parametrize('kernel,family,mutate', TN_MUTATION_GRID, ids=['-'.join(c) for c in TN_MUTATION_GRID])
def test_tn_mutations_are_rejected(kernel, family, mutate):
    """At the smallest case of the kernel's grid on which the corruption can happen (two non-empty chunks for a row in the neighbouring chunk, a second row tile for the
    bias of the wrong tile, an empty chunk for the unwritten one)."""
    cases = T.TN_SPLITK_CASES if kernel == 'splitk' else T.TN_PP_CASES
    tile = T.TN_TILE[kernel]
    need = {'neighbour_chunk': lambda f, M, N, K, s, kc: M > kc, 'bias_tile1': lambda f, M, N, K, s, kc: N > tile,
            'empty_unwritten': lambda f, M, N, K, s, kc: (s - 1) * kc >= M, 'swap_chunks': lambda f, M, N, K, s, kc: M >= 2,
            'read_row_M': lambda f, M, N, K, s, kc: M % kc != 0}.get(mutate, lambda *a: True)
    fam, M, N, K, split, kc = _first(cases, lambda f, *a: f == family and need(f, *a))
    dy, x = T.tn_operands(fam, M, N, K, seed=M + N)
    part, bias = T.tn_emulate(kernel, dy, x, M, split, kc, mutate=mutate)
    msgs = T.tn_verdict(kernel, fam, dy, x, M, split, kc, part, bias)
    assert msgs, f'{mutate} passed at {(fam, M, N, K, split, kc)}'
    if mutate == 'bias_tile1':
        assert all(m.startswith('bias_part') for m in msgs), msgs


def test_marker_names_the_token_rows():
    fam, M, N, K, split, kc = T.TN_SPLITK_CASES[-1]
    assert fam == 'marker'
    dy, x = T.tn_operands(fam, M, N, K, seed=0)
    part, bias = T.tn_emulate('splitk', dy, x, M, split, kc, mutate='neighbour_chunk')
    msgs = T.tn_verdict('splitk', fam, dy, x, M, split, kc, part, bias)
    # token row 192 (= kc: the first row of chunk 1, output row 192 % 128 = 64) was counted in chunk 0 instead
    assert 'chunk 0 output row 64 (token rows [64]): codes got [258.0, 2.0] want [65.0, 1.0]' in msgs, msgs
    assert 'chunk 1 output row 64 (token rows [192]): codes got [0.0, 0.0] want [193.0, 1.0]' in msgs, msgs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the other kernels: the emulation passes, the corruption fails (smallest case of each grid)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _softmax_buffers(S, scale, L_pad, mutate=None):
    rows = S.shape[0]
    pre = G.canary((rows, L_pad + 8), torch.bfloat16)
    got = pre.clone()
    got[:, :L_pad] = T.softmax_emulate(S, scale, L_pad, mutate)
    return got, pre


@pytest.mark.parametrize('kind', T.SOFTMAX_KINDS)
@pytest.mark.parametrize('L', [1, 65, 256])
def test_softmax_emulation_passes(kind, L):
    for scale in T.SOFTMAX_SCALES:
        S = T.softmax_logits(kind, 5, L, scale, seed=L)
        for L_pad in T.softmax_lpads(L):
            got, pre = _softmax_buffers(S, scale, L_pad)
            assert T.softmax_verdict(S, scale, L_pad, got, pre) == []
            P = got[:, :L].clone()
            dP = T.softmax_bwd_dp(P, seed=L)                        # rows 0 / 3 Gaussian, 1 / 4 constant, 2 with a cancelling dot product
            pd = (P.double() * dP.double())[2]
            assert L == 1 or abs(float(pd.sum())) <= 1e-6 * float(pd.abs().sum()) and float(pd.abs().sum()) >= L - 1.001
            gb = pre.clone()
            gb[:, :L_pad] = T.softmax_bwd_emulate(P, dP, scale, L_pad)
            assert T.softmax_bwd_verdict(P, dP, scale, L_pad, gb, pre) == []


@pytest.mark.parametrize('mutate,kind', [('no_max', 'shifted'), ('norm_lpad', 'flat'), ('rtz', 'spread')])
def test_softmax_mutations_are_rejected(mutate, kind):
    L, L_pad = 63, 64                                              # the smallest L with a pad column
    S = T.softmax_logits(kind, 1, L, 1.0, seed=1)
    got, pre = _softmax_buffers(S, 1.0, L_pad, mutate)
    assert T.softmax_verdict(S, 1.0, L_pad, got, pre)
    got, pre = _softmax_buffers(S, 1.0, L_pad)
    got[0, L_pad] = 0.0                                            # and a write behind L_pad
    assert T.softmax_verdict(S, 1.0, L_pad, got, pre)


def test_softmax_bwd_mutation_and_cancellation():
    """The row whose dot product cancels (sum p dP ~ 1e-8 sum |p dP|) passes as emulated; an emulation whose dot product misses one term - an error of 1 / L of
    sum |p dP|, nothing next to |dP| = 1 / p - fails on exactly that row, and on a Gaussian row."""
    L = 64
    pre = G.canary((3, L + 8), torch.bfloat16)
    for kind in ('flat', 'spread'):
        P = T.softmax_emulate(T.softmax_logits(kind, 3, L, 1.0, seed=2), 1.0, L)
        dP = T.softmax_bwd_dp(P, seed=3)
        got = pre.clone()
        got[:, :L] = T.softmax_bwd_emulate(P, dP, 1.0, L)
        assert T.softmax_bwd_verdict(P, dP, 1.0, L, got, pre) == []
        if kind == 'flat':
            got[:, :L] = T.softmax_bwd_emulate(P, dP, 1.0, L, mutate='drop_last_term')
            for r in (0, 2):
                assert T.softmax_bwd_verdict(P[r:r + 1], dP[r:r + 1], 1.0, L, got[r:r + 1], pre[r:r + 1]), f'row {r}'


@pytest.mark.parametrize('bf16', [False, True])
def test_colsum_emulation_and_mutation(bf16):
    rows, cols = 65, 21                                            # the smallest case with a second (partial) block
    x = torch.randn(rows, cols, generator=G.gen(4))
    x = x.bfloat16() if bf16 else x
    pre = torch.randn(cols, generator=G.gen(5))
    for acc in (False, True):
        for vec in (False, True):
            got = T.colsum_emulate(x) + (pre if acc else 0.0)
            assert T.colsum_verdict(x, pre, acc, vec, got) == []
            assert T.colsum_verdict(x, pre, acc, vec, T.colsum_emulate(x, 'drop_last_block') + (pre if acc else 0.0))
    assert T.colsum_depth(16383, False) > T.colsum_depth(16383, True) and T.colsum_rpb(16384) == 256 and T.colsum_workspace(65, 21) == 42


@pytest.mark.parametrize('kind', T.CE_KINDS)
def test_cross_entropy_emulation_and_mutation(kind):
    for B, C in ((1, 1), (1, 2), (16, 21), (33, 130)):
        z, tgt = T.ce_logits(kind, B, C, seed=B + C)
        for gs in (1.0, 0.25):
            loss, grad = T.ce_emulate(z, tgt, gs)
            assert T.ce_verdict(z, tgt, gs, loss, grad) == [] and T.ce_verdict(z, tgt, gs, loss, None) == []
    z, tgt = T.ce_logits(kind, 16, 2, seed=1)                      # the smallest case with B > 1 and a non-zero gradient
    loss, grad = T.ce_emulate(z, tgt, 1.0, mutate='no_div_B')
    assert T.ce_verdict(z, tgt, 1.0, loss, grad)


def _adam_case(n, seed):
    g = G.gen(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-6


@pytest.mark.parametrize('step', T.ADAM_STEPS)
def test_adam_emulation_and_mutations(step):
    p, g, m, v = _adam_case(255, step)
    norm = g.double().norm().float()
    for max_norm in (0.0, 100.0, 1.0, float(norm)):               # no clipping, inactive, active, at the threshold
        pn, mn, vn = T.adam_emulate(p, g, m, v, norm, max_norm, step)
        assert T.adam_verdict(p, g, m, v, norm, max_norm, step, pn, mn, vn, pn.bfloat16()) == []
        assert T.adam_verdict(p, g, m, v, norm, max_norm, step, pn, mn, vn, G.round_bf16(pn, rtz=True).bfloat16())
    p, g, m, v = _adam_case(1, step)                               # the smallest case
    norm = torch.tensor(abs(float(g[0])) * 4 + 1.0)
    if step < 100000:                                              # (at step 100000 both corrections are 1 in fp32 and in float64: nothing to swap)
        assert T.adam_verdict(p, g, m, v, norm, 1.0, step, *T.adam_emulate(p, g, m, v, norm, 1.0, step, mutate='swap_bc'), None)
    assert T.adam_verdict(p, g, m, v, norm, 1.0, step, *T.adam_emulate(p, g, m, v, norm, 1.0, step, mutate='clip_after'), None)


def test_meanpool_emulation_and_mutation():
    g = G.gen(6)
    for n, t in ((1, 1), (3, 6), (5, 8)):
        for mag in (1e-14, 1.0, 1e14):                            # pooled-row norms ~ 28 mag / sqrt(t): inside [1e-15, 1e15]
            x = torch.randn(n * t, 768, generator=g) * mag
            x[:t] = 0.0 if n > 1 else x[:t]                         # an all-zero group
            for normalize in (0, 1):
                y, bar = T.meanpool_reference(x, t, normalize)
                got = T.meanpool_emulate(x, t, normalize)
                assert T.within(got, y, bar, 'meanpool') == []
                if n > 1:
                    assert float(got[0].abs().max()) == 0.0 and float(y[0].abs().max()) == 0.0
    x = torch.randn(1, 768, generator=g)                           # the smallest case; normalisation would hide the factor, so normalize = 0
    y, bar = T.meanpool_reference(x, 1, 0)
    assert T.within(T.meanpool_emulate(x, 1, 0, mutate='t_plus_1'), y, bar, 'meanpool')


def test_similarity_emulation_and_mutation():
    for family in ('exact', 'wide'):
        for scale in T.SIM_SCALES:
            a, b = T.sim_operands(family, 1, 1, 16, seed=7)        # the smallest case
            pre = G.canary((3, 4), torch.float32)
            assert T.sim_verdict(family, a, b, scale, T.sim_emulate(a, b, scale, 3, 4), pre) == []
            assert T.sim_verdict(family, a, b, scale, T.sim_emulate(a, b, scale, 3, 4, mutate='write_past_n'), pre)
            a, b = T.sim_operands(family, 65, 130, 768, seed=8)
            assert T.sim_verdict(family, a, b, scale, T.sim_emulate(a, b, scale, 66, 136), G.canary((66, 136), torch.float32)) == []


def test_shift_preds_data_discriminates():
    """Every clip of every case is a random integer block with the ties planted into it: the expected predictions differ between the two directions and between the
    clips, and each corruption - the last maximum on a tie, the two outputs swapped, windows of W - 1 terms, the next clip's block - changes them."""
    for (S, W) in T.SHIFT_CASES:
        n = S - W + 1
        for n_clips in (1, 3):
            Gm = T.shift_operands(n_clips, S, W, n_clips * S + 4, seed=T.shift_seed(S, W))
            blocks = torch.block_diag(*[torch.ones(S, S)] * n_clips).bool()
            inside = Gm[:, :n_clips * S][blocks]
            assert float(inside.abs().max()) <= 8 and inside.equal(inside.round()) and inside.unique().numel() >= 8
            assert float(Gm[:, :n_clips * S][~blocks].min() if n_clips > 1 else 1e30) > 1e29 and float(Gm[:, n_clips * S:].min()) > 1e29
            pa, pv = T.shift_reference(Gm, n_clips, S, W)
            assert T.shift_verdict(Gm, n_clips, S, W, pa, pv) == []
            if n == 1:
                continue                                            # a single shift: nothing to decide
            assert not pa.equal(pv) and T.shift_verdict(Gm, n_clips, S, W, pv, pa), 'the two directions agree'
            if n >= 3:
                assert (pv[:, 0] == 1).all() and (pa[:, n - 1] == 0).all()      # the planted ties: the first of the two maxima
            muts = ['last', 'short_window'] + (['next_clip'] if n_clips > 1 else [])
            for mutate in muts:
                assert T.shift_verdict(Gm, n_clips, S, W, *T.shift_reference(Gm, n_clips, S, W, mutate=mutate)), f'{mutate} passed at S {S} W {W} clips {n_clips}'
            if n_clips > 1:
                assert not pa[0].equal(pa[1]) or not pv[0].equal(pv[1])
    Gm = T.shift_operands(1, 5, 3, 5, seed=T.shift_seed(5, 3))     # the smallest case
    la, lv = T.shift_reference(Gm, 1, 5, 3, mutate='last')
    assert int(la[0, 2]) == 2 and int(lv[0, 0]) == 2 and T.shift_verdict(Gm, 1, 5, 3, la, lv)


def test_reduce_groups_emulation_and_mutation():
    g = G.gen(9)
    for Gn, cols in ((1, 8), (7, 60), (196, 520)):
        x = torch.randn(3, Gn, cols, generator=g).bfloat16()
        pre = torch.randn(3, cols, generator=g).bfloat16()
        for acc in (False, True):
            for vec in (False, True):
                assert T.reduce_groups_verdict(x, pre, acc, vec, T.reduce_groups_emulate(x, pre, acc)) == []
                if Gn > 1:
                    assert T.reduce_groups_verdict(x, pre, acc, vec, T.reduce_groups_emulate(x, pre, acc, mutate='missing_last_group'))
    x = torch.randn(1, 1, 8, generator=g).bfloat16()               # the smallest case: G = 1, the missing group is the only one
    assert T.reduce_groups_verdict(x, x[:, 0], False, False, torch.zeros(1, 8).bfloat16())
