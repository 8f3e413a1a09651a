"""CPU: the harness of tests/test_rowops_fwd_gpu.py is itself right, and would reject a subtly wrong kernel.  Each reference of tests/rowops_fwd_oracle.py is
checked against an independent restatement (gemm_oracle.mx_quant_ref and torch's float8 cast, torch's bf16 cast, oracle.rgb_frontend, oracle.token_mask_from_content,
the float64 definitions of the mel tables and oracle.mel_filterbank, torch.stft); the fp32 emulations of a correct kernel must pass every criterion at the margins
the bars were written for; and the emulated defects - a one-pass variance, a row dropped at rows % 4, a scale byte in the neighbouring plane, the round-up scale
rule, truncation instead of round-to-nearest-even, the mel reflection off by one, fb_hi one too small, a token mask that ignores zero weights, two patch-rows
swapped - must each be rejected."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402
import rowops_fwd_oracle as R  # noqa: E402

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', R.LN_EPS)
@pytest.mark.parametrize('family', R.LN_FAMILIES)
def test_layernorm_emulation_within_bar(family, eps):
    """The emulation in the kernel's order uses a small part of the bar for the plain fp32 output (below 0.06 on every family and eps; 0.25 is asserted) and passes
    the accumulated and the bf16 one - there the output's own rounding may take all of its term (half an ulp of a sum is up to 2^-24 (|prefill| + |y|))."""
    x = R.ln_input(family, 37, seed=3)
    g, b = R.ln_params(4)
    pre = torch.randn(37, R.D, generator=G.gen(5)) * 2
    for out_bf16, prefill in ((False, None), (False, pre), (True, None)):
        ref, bar = R.ln_expected(x, g, b, eps, out_bf16, prefill)
        res = R.elem_check(R.ln_emulate(x, g, b, eps, out_bf16, prefill), ref, bar)
        assert res['msg'] is None, res['msg']
        assert out_bf16 or prefill is not None or res['worst'] < 0.25, res['worst']


def test_layernorm_one_pass_variance_rejected():
    """var = E[x^2] - mean^2 misses the fp32 bar about tenfold on the offset-100 family (a bf16 output's own ulp hides three lost digits: that output is held by
    the offset-1e4 family, where the one-pass variance is rounding noise of either sign)."""
    g, b = R.ln_params(4)
    for family, out_bf16, least in (('offset100', False, 3.0), ('offset1e4', False, 100.0), ('offset1e4', True, 100.0)):
        x = R.ln_input(family, 37, seed=3)
        ref, bar = R.ln_expected(x, g, b, 1e-6, out_bf16)
        res = R.elem_check(R.ln_emulate(x, g, b, 1e-6, out_bf16, one_pass=True), ref, bar)
        assert res['msg'] is not None and res['worst'] > least, (family, out_bf16, res['worst'])


def test_constant_rows_need_the_mean_term():
    """A constant row's variance is exactly 0 and the reference is beta.  A mean one ulp off is amplified by rstd, up to 1e6 at eps 1e-12: only the bar's third term
    admits that, and it must (fl(1 / 768) * 768 is not 1, so no order of operations is obliged to return the constant); a mean 64 ulp off is still rejected."""
    x = R.ln_input('const', 9, seed=0)
    g, b = R.ln_params(4)
    ref, bar = R.ln_expected(x, g, b, 1e-12, False)
    assert torch.equal(ref, b.double().unsqueeze(0).expand(9, -1))
    assert R.elem_check(R.ln_emulate(x, g, b, 1e-12), ref, bar)['msg'] is None
    rstd = 1e6
    for ulps, ok in ((1, True), (200, False)):
        off = ulps * 2.0 ** -24 * x.double().abs()                    # x - mean when the mean is `ulps` units of 2^-24 |mean| off, variance off^2 << eps
        got = off * rstd * g.double() + b.double()
        assert (R.elem_check(got, ref, bar)['msg'] is None) == ok, ulps


@pytest.mark.parametrize('rows', [5, 6, 7, 9])
def test_dropped_tail_rows_rejected(rows):
    """A kernel that skips the rows behind the last whole group of 4 leaves the canary there: NaN in a float output, foreign bytes in a byte output."""
    x = R.ln_input('gauss', rows, seed=1)
    g, b = R.ln_params(4)
    ref, bar = R.ln_expected(x, g, b, 1e-6, False)
    pre = G.canary((rows, R.D), F32)
    assert R.elem_check(R.drop_tail_rows(R.ln_emulate(x, g, b, 1e-6), pre, rows), ref, bar)['msg'] is not None
    want = R.rne_bf16_bits(x)
    assert R.bits_mismatch(R.drop_tail_rows(want, G.canary((rows, R.D), BF16), rows), want) is not None
    xb = R.mx_matrix(R.mx_blocks(), rows, 128)
    q, _ = R.mx_quant_int(xb)
    assert R.bits_mismatch(R.drop_tail_rows(q, G.canary((rows, 128), U8), rows), q) is not None


def test_row_maps():
    """map_rows restates sf_common.h's map_row; the engine's two maps are injective onto the rows the tests expect."""
    m = (1568, 196, 8 * 197, 197, 1, 1)
    o = R.map_rows(m, 1568)
    assert o.unique().numel() == 1568 and not (o % 197 == 0).any() and int(o.max()) == 8 * 197 - 1
    assert torch.equal(R.map_rows((1568, 1568, 1569, 0, 1, 1), 1568), torch.arange(1, 1569))
    o = R.map_rows((72, 6, 78, 1, 13, 1), 144)
    assert o.unique().numel() == 144 and not (o % 13 == 0).any()
    assert int(o[7]) == 1 * 1 + 1 * 13 + 1                  # r = 7: fi = 1, ti = 1 -> row ti * 13 + 1 + fi


# ---- MXFP8 -------------------------------------------------------------------------------------------------------------------------------------------
def test_e4m3_rounding_equals_torch_cast():
    """Every bf16 significand (normal: 128 + m, subnormal: m) at every scale that lands it inside (-448, 448) - all the values a scaled bf16 element can take - and
    both signs: the integer rounding equals torch's float8_e4m3fn cast.  Then every one of the 2^16 bf16 patterns itself, those inside (-448, 448)."""
    M = torch.arange(256).repeat_interleave(40)
    s = (torch.arange(40) - 36).repeat(256)                   # 2^-36 .. 2^3
    v = M.double() * torch.exp2(s.double())
    ok = v < 448
    for sign in (0, 1):
        f = (v * (1 - 2 * sign)).float()
        want = f.to(torch.float8_e4m3fn).view(U8)
        got = R.e4m3_bits(torch.full_like(M, sign), M, s).to(U8)
        assert torch.equal(got[ok], want[ok])
    allb = torch.arange(1 << 16).to(torch.int16).view(BF16)
    fin = torch.isfinite(allb.float()) & (allb.float().abs() < 448)
    sign, Mb, E, _ = R.bf16_fields(allb)
    assert torch.equal((Mb.double() * torch.exp2(E.double()) * (1 - 2 * sign))[fin], allb.double()[fin])
    assert torch.equal(R.e4m3_bits(sign, Mb, E).to(U8)[fin], allb.float().to(torch.float8_e4m3fn).view(U8)[fin])
    assert int(R.e4m3_bits(torch.tensor(0), torch.tensor(255), torch.tensor(1))) == 0x7E        # 510 saturates to 448
    assert int(R.e4m3_bits(torch.tensor(1), torch.tensor(1), torch.tensor(-30))) == 0x80        # underflow keeps the sign


def test_mx_oracle_equals_restatement():
    """mx_quant_int == gemm_oracle.mx_quant_ref (floor(log2), fp32 scaling, torch's cast) on the constructed blocks, on Gaussian rows and on all finite bf16 patterns
    grouped by magnitude (so that a block's elements survive its scale) and at random."""
    blocks = R.mx_blocks()
    cases = [R.mx_matrix(blocks, blocks.shape[0], 32), (torch.randn(64, 256, generator=G.gen(1)) * 3).bfloat16()]
    allb = torch.arange(1 << 16).to(torch.int16).view(BF16)
    fin = allb[torch.isfinite(allb.float())]
    fin = fin[: fin.numel() // 32 * 32]
    cases.append(fin[fin.float().abs().argsort()].view(-1, 32))
    cases.append(fin[torch.randperm(fin.numel(), generator=G.gen(2))].view(-1, 128))
    for x in cases:
        q, sc = R.mx_quant_int(x)
        qr, scr = G.mx_quant_ref(x)
        assert torch.equal(sc, scr) and torch.equal(q, qr)


def test_mx_blocks_cover_the_edges():
    blocks = R.mx_blocks()
    x = R.mx_matrix(blocks, blocks.shape[0], 32)
    q, sc = R.mx_quant_int(x)
    mag = q & 0x7F
    assert int(sc.min()) == 1 and int(sc.max()) == 246                                     # the lower clamp (zero, subnormal and 2^-126 .. blocks) and 2^127
    assert (mag == 0x7E).any() and ((mag > 0) & (mag < 8)).any() and (q == 0x80).any() and (q == 0).any()      # saturation, e4m3 subnormals, -0, +0
    assert (q[-2] == 0).all() and int(sc[-2]) == 1 and set(q[-1].tolist()) == {0, 0x80} and int(sc[-1]) == 1   # the all-zero blocks
    sign, M, E, _ = R.bf16_fields(x)
    s = E + 127 - sc.long().repeat_interleave(32, 1)
    r = (-6 - 3 - s).clamp(1, 40)                                                         # ties in the subnormal range: the bits below the step are exactly one half
    assert ((M > 0) & (s < -9) & ((M & ((1 << r) - 1)) == (1 << (r - 1)))).any()
    sc4 = sc[:2436].view(-1, 12)
    assert torch.equal(G.mx_unplane(G.mx_planes(sc4, sc4.shape[0] + 3), sc4.shape[0]), sc4)


def test_mx_defects_rejected():
    blocks = R.mx_blocks()
    x = R.mx_matrix(blocks, 70, 3072)
    q, sc = R.mx_quant_int(x)
    q1, sc1 = R.mx_quant_int(x, rule=1)
    assert not torch.equal(sc1, sc) and not torch.equal(q1, q)                             # the round-up scale rule
    qt, sct = R.mx_quant_int(x, truncate=True)
    assert torch.equal(sct, sc) and not torch.equal(qt, q)                                 # truncation instead of RNE
    planes = G.mx_planes(sc, 73)
    assert not torch.equal(G.mx_unplane(planes.roll(1, 0), 70), sc)                        # a scale byte in the neighbouring plane
    assert not torch.equal(G.mx_unplane(planes.roll(1, 2), 70), sc)                        # ... or at the neighbouring byte of its dword
    g = (torch.randn(8, 256, generator=G.gen(1)) * 3).bfloat16()                           # Gaussian rows too: a fifth of the blocks has a mantissa above 1.75
    assert not torch.equal(R.mx_quant_int(g, rule=1)[1], R.mx_quant_int(g)[1])


# ---- moves -------------------------------------------------------------------------------------------------------------------------------------------
def test_rne_bf16_equals_torch():
    x = R.f32_probes((64, R.D), 7)
    assert not torch.isnan(x).any() and torch.isinf(x).any() and ((x != 0) & (x.abs() < 2.0 ** -126)).any()
    lo = G.bits(x).to(torch.int64) & 0xFFFF
    assert all(((lo == v).any() for v in (0x8000, 0x7FFF, 0x8001)))
    assert R.bits_mismatch(R.rne_bf16_bits(x), x.bfloat16()) is None
    trunc = (G.bits(x).to(torch.int64) >> 16).to(torch.int16).view(BF16)
    assert R.bits_mismatch(trunc, R.rne_bf16_bits(x)) is not None                          # truncation instead of RNE


# ---- patch gathers -----------------------------------------------------------------------------------------------------------------------------------
def test_u8_table_equals_rgb_frontend():
    from oracle import synchformer_cpu as O
    b = torch.arange(256, dtype=U8)
    assert R.bits_mismatch(R.u8_table(), O.rgb_frontend(b).bfloat16()) is None
    assert len(set(G.bits(R.u8_table()).tolist())) > 200


def test_patch_maps_and_swapped_rows():
    """video_patches / spec_patches put element (n, t, c, y, x) where the kernels' comments say; two swapped patch-rows are seen."""
    x = torch.arange(2 * 16 * 3 * 224 * 224, dtype=torch.int32).reshape(2, 16, 3, 224, 224)
    p = R.video_patches(x)
    g = G.gen(3)
    for _ in range(200):
        n, f, h, w, c, dt, dh, dw = (int(torch.randint(0, k, (1,), generator=g)) for k in (2, 8, 14, 14, 3, 2, 16, 16))
        assert int(p[n * 1568 + f * 196 + h * 14 + w, ((c * 2 + dt) * 16 + dh) * 16 + dw]) == int(x[n, f * 2 + dt, c, h * 16 + dh, w * 16 + dw])
    assert not torch.equal(R.swap_patch_rows(p), p)
    clips = torch.arange(2 * 23, dtype=torch.int32).view(2, 23, 1, 1, 1).expand(2, 23, 3, 2, 2)
    seg = R.clip_segments(clips, 3, 4, 2)
    assert seg.shape[:2] == (4, 16) and seg[:, 0, 0, 0, 0].tolist() == [3, 7, 26, 30] and int(seg[3, 15, 0, 0, 0]) == 45
    for F, Ta in ((128, 66), (16, 16), (37, 29), (26, 17)):
        s = torch.arange(3 * F * Ta, dtype=torch.int32).reshape(3, F, Ta)
        nf, nt = (F - 16) // 10 + 1, (Ta - 16) // 10 + 1
        q = R.spec_patches(s)
        assert q.shape == (3 * nf * nt, 256)
        assert int(q[(2 * nf + nf - 1) * nt + nt - 1, 5 * 16 + 9]) == int(s[2, 10 * (nf - 1) + 5, 10 * (nt - 1) + 9])


def test_video_inputs_hold_the_edge_values():
    for dtype in (U8, torch.float16, BF16, F32):
        vid, want = R.video_input(dtype, (3, 224, 224), 5)
        assert vid.dtype == dtype and want.dtype == BF16 and not torch.isnan(want.float()).any()
        if dtype == U8:
            assert vid.unique().numel() == 256
        elif dtype != BF16:
            assert R.bits_mismatch(want, vid.float().bfloat16()) is None
            low = G.bits(vid.float()).to(torch.int64) & 0xFFFF
            assert (low == 0x8000).any()                                                  # values on bf16 ties
        if dtype == torch.float16:
            assert (vid.float().abs() == 65504).any() and ((vid != 0) & (vid.float().abs() < 2.0 ** -14)).any()


# ---- token masks -------------------------------------------------------------------------------------------------------------------------------------
def test_token_mask_rule_and_cases():
    from oracle import synchformer_cpu as O
    w0s = R.video_w0_sign()
    assert set(w0s.tolist()) == {1, -1, 0}
    w0 = w0s.double() * (0.5 + torch.rand(1536, generator=G.gen(1)).double())
    keep, want = R.video_mask_cases(2)
    pk = R.video_patches(keep).view(2, 1568, 1536)
    lit = R.token_keep_literal(pk, w0)
    assert torch.equal(lit, O.token_mask_from_content(pk, w0))
    assert torch.equal(lit.to(U8), want[:, 1:]) and (want[:, 0] == 1).all()
    assert 0 < int((want == 0).sum()) < 2 * len(R.V_TOKENS) and not torch.equal(want[0], want[1])
    assert not torch.equal(R.token_keep_no_zero(pk, w0), lit)                             # a mask that ignores zero weights
    rnd = torch.rand(2, 1568, 1536, generator=G.gen(2)) > 0.0005                          # and on random masks
    assert torch.equal(R.token_keep_literal(rnd, w0), O.token_mask_from_content(rnd, w0))
    ws = R.spec_w0_sign()
    for i, (F, Ta) in enumerate(((128, 66), (16, 16), (37, 29), (26, 17))):
        k = R.spec_mask_cases(2, F, Ta, seed=i)
        got = R.spec_token_keep(k, ws)
        ref = O.token_mask_from_content(R.spec_patches(k).view(2, -1, 256), ws.double())
        assert torch.equal(got[:, 2:].bool(), ref) and (got[:, :2] == 1).all()


# ---- mel front-end -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tables():
    from synchformer_amd import frontend
    return {n: frontend.mel_tables(n) for n in (128, 40)}


def test_mel_tables(tables):
    """The fp32 tables the kernel reads are their float64 definitions rounded once; fb (n_mels = 40 and 128) equals oracle.mel_filterbank; [fb_lo, fb_hi) is each
    filter's support exactly."""
    from oracle import synchformer_cpu as O
    t = tables[128]
    n, k = np.arange(400, dtype=np.float64), np.arange(513, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 400)
    ang = 2 * np.pi * np.outer(312 + n, k) / 1024
    for name, want in (('tw_cos', hann[:, None] * np.cos(ang)), ('tw_sin', -hann[:, None] * np.sin(ang))):
        assert t[name].dtype == np.float32 and t[name].shape == (400, 513)
        assert (np.abs(t[name].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-45).all()
    assert np.array_equal(tables[40]['tw_cos'], t['tw_cos'])
    for n_mels in (128, 40):
        fb = tables[n_mels]['fb']
        assert fb.shape == (513, n_mels) and fb.dtype == np.float32 and (fb >= 0).all()
        np.testing.assert_allclose(fb, O.mel_filterbank(n_mels=n_mels).numpy(), rtol=0, atol=1e-7)
        lo, hi = tables[n_mels]['fb_lo'], tables[n_mels]['fb_hi']
        for j in range(n_mels):
            nz = np.nonzero(fb[:, j])[0]
            assert nz.size and lo[j] == nz[0] and hi[j] == nz[-1] + 1


def test_mel_reference_equals_stft(tables):
    """The float64 reference against the oracle's torch.stft restatement (fp32): the frames, the reflection, the filterbank, the log, the padding and the
    truncation at pad_to.  Wherever the bar is not vacuous the difference is a small multiple of it (torch's fp32 FFT is not the kernel's order: 20 bars)."""
    from oracle import synchformer_cpu as O
    from synchformer_amd.frontend import AST_MEAN, AST_STD
    for n in (513, 5000, 10560, 11111):
        w = R.mel_wave('noise', 2, n, seed=n)
        exp = R.mel_reference(w, tables[128], 66, AST_MEAN, AST_STD)
        assert exp['frames'] == min(n // 160 + 1, 66)
        stft = O.mel_frontend(w)[:, 0].double()
        assert float((stft - exp['ref']).abs().max()) < 2e-4


@pytest.mark.parametrize('family', R.MEL_FAMILIES)
def test_mel_emulation_within_bar(tables, family):
    """The emulation in the kernel's order: the non-tonal families stay within 0.3 of a bar that never exceeds the cap (0.14 and 1.8e-3 were measured when the bar
    was written); the tonal ones pass the elementwise criterion wherever the bar holds, and - against themselves - the per-frame one."""
    from synchformer_amd.frontend import AST_MEAN, AST_STD
    for n, n_mels in ((5000, 128), (513, 40)):
        w = R.mel_wave(family, 2, n, seed=11)
        exp = R.mel_reference(w, tables[n_mels], 66, AST_MEAN, AST_STD)
        emu = R.mel_emulate(w, tables[n_mels], 66, AST_MEAN, AST_STD)
        tonal = family in R.MEL_TONAL
        res = R.mel_check(emu, exp, emu if tonal else None)
        assert res['msg'] is None, res['msg']
        if not tonal:
            assert float(exp['bar'].max()) < R.MEL_CAP and res['worst'] < 0.3, (float(exp['bar'].max()), res['worst'])
        else:
            assert 0 < res['share'] < 1, res['share']                                      # the cap does divide a tonal output


@pytest.mark.parametrize('family', ['noise', 'impulse0', 'impulse_last', 'tone440'])
@pytest.mark.parametrize('defect', ['symmetric', 'hi_short'])
def test_mel_defects_rejected(tables, family, defect):
    """The reflection off by one (the edge sample repeated) and fb_hi one too small.  An impulse at either end shows the reflection alone: the frames that see the
    edge miss by O(0.5).  A lost last bin of every filter is seen in every family."""
    from synchformer_amd.frontend import AST_MEAN, AST_STD
    n = 5000
    w = R.mel_wave(family, 2, n, seed=11)
    exp = R.mel_reference(w, tables[128], 66, AST_MEAN, AST_STD)
    emu = R.mel_emulate(w, tables[128], 66, AST_MEAN, AST_STD)
    bad = R.mel_emulate(w, tables[128], 66, AST_MEAN, AST_STD, **{defect: True})
    tonal = family in R.MEL_TONAL
    res = R.mel_check(bad, exp, emu if tonal else None)
    assert res['msg'] is not None
    if family.startswith('impulse') and defect == 'symmetric':
        assert float((bad.double() - exp['ref']).abs().max()) > 0.05
    pad = bad.clone()
    pad[:, :, exp['frames']:] += 2.0 ** -20                                                # a padded frame one ulp off is seen
    assert R.mel_check(pad, exp, emu if tonal else None)['msg'] is not None
