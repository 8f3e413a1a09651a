"""GPU: the weight-gradient GEMMs sf_gemm_tn_splitk (sf_gemm.hip) and sf_gemm_tn_pp (sf_gemm_tn_pp.hip) against float64 computed from the very bf16 values the
kernels read.  Grids, references, emulation and bars are tests/train_tail_oracle.py's (tests/test_train_tail_oracle_cpu.py shows that they reject a subtly wrong
kernel); conventions are those of tests/test_gemm_gpu.py:
  exact   integer operands (dY in [-4, 4], X in [-8, 8], every partial sum below 2^24): part and bias_part BIT FOR BIT equal to the int64 result, whatever the
          chunking, ring order or swizzle;
  marker  dY[m, i] = 1 iff i == m mod N, X a code of the token row: bit for bit, and a failure names the token rows behind the wrong outputs;
  wide    Gaussian operands whose magnitude changes per 32-token block and per column: elementwise  |got - ref| <= MARGIN (d + 2) 2^-24 sum |dy x|  and, per 64 x 64
          block, ||got - ref|| <= STAT_FACTOR ||emu - ref|| + ||F||, emu accumulating the kernel's MFMA k-steps (32 tokens in tn_splitk, 16 in tn_pp) in fp32.
  d (longest chain of dependent fp32 additions):  tn_splitk part AND bias_part kc / 32 + 32 (one v_mfma_f32_16x16x32_bf16 per 32-token stage in the kt loop of
  gemm_tn_splitk_kernel into acc[][] and, against all-ones, into accb[]);  tn_pp part kc / 16 + 16 (mma(): four v_mfma_f32_32x32x16_bf16 k-steps per phase into each
  acc[][]), bias_part kc / 2 + 1 (bias_acc(): per k-tile 4 fragments x 4 v_dot2_f32_bf16, two additions each, into one bsum[] per lane, + the __shfl_xor(32) add).
Every case: rows of dY and X beyond M hold NaN, both operands are column slices of wider buffers (the rest NaN), part and bias_part start as position-dependent
canaries with more canary behind them, and the launch is made with and without bias_part - part must be bit-identical between the two.  Refusals are asserted through
the return code of the launcher's argument check (nothing is launched).

Measured on an MI355X (gfx950, 256 CUs: sf_gemm_tn_pp launches 256 workgroups, the walks run 261 and 521 items): 23 tests, 3.8 s (the two walks 0.6 s each).  Every
exact, marker and walk case bit for bit, repetitions identical, no bug found.  wide, worst error / bar and worst block ratio:  tn_splitk part 0.077 / 0.011, bias_part
0.017 / 0.0032;  tn_pp part 0.117 / 0.013, bias_part 0.0074 / 0.0014."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402
import train_tail_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from synchformer_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fn(kernel):
    return _lib().sf_gemm_tn_splitk if kernel == 'splitk' else _lib().sf_gemm_tn_pp


def _upload(dy, x, dev):
    """The operands as column slices of wider NaN buffers on the device: dY = buf[:, 64:], X = buf[:, :K]."""
    dyw = torch.full((dy.shape[0], dy.shape[1] + T.TN_LD_EXTRA[0]), float('nan'), dtype=torch.bfloat16)
    xw = torch.full((x.shape[0], x.shape[1] + T.TN_LD_EXTRA[1]), float('nan'), dtype=torch.bfloat16)
    dyw[:, T.TN_LD_EXTRA[0]:], xw[:, :x.shape[1]] = dy, x
    dyw, xw = dyw.to(dev), xw.to(dev)
    return dyw[:, T.TN_LD_EXTRA[0]:], xw[:, :x.shape[1]]


TAIL = 96       # canary floats behind part and behind bias_part


def _launch(kernel, dyd, xd, M, N, K, split, kc, with_bias, pre_p, pre_b):
    """One launch into fresh copies of the canary buffers; returns part (split, N, K), bias_part (split, N) or None, after asserting the canaries behind them."""
    pb, bb = pre_p.clone(), pre_b.clone()
    rc = _fn(kernel)(dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), pb.data_ptr(), bb.data_ptr() if with_bias else None, M, N, K, split, kc, _st())
    from synchformer_amd import _lib as L
    L.check(rc, f'sf_gemm_tn_{kernel}')
    torch.cuda.synchronize()
    n_p, n_b = split * N * K, split * N
    assert torch.equal(G.bits(pb[n_p:]), G.bits(pre_p[n_p:])), 'written behind part'
    assert torch.equal(G.bits(bb[n_b if with_bias else 0:]), G.bits(pre_b[n_b if with_bias else 0:])), 'written behind bias_part (or into it without being asked)'
    return pb[:n_p].view(split, N, K), bb[:n_b].view(split, N) if with_bias else None


def _run_case(kernel, gpu, family, M, N, K, split, kc, stats):
    dy, x = T.tn_operands(family, M, N, K, seed=M + N)
    dyd, xd = _upload(dy, x, gpu)
    pre_p = G.canary((split * N * K + TAIL,), torch.float32).to(gpu)
    pre_b = G.canary((split * N + TAIL,), torch.float32).to(gpu)
    part, bias = _launch(kernel, dyd, xd, M, N, K, split, kc, True, pre_p, pre_b)
    part0, _ = _launch(kernel, dyd, xd, M, N, K, split, kc, False, pre_p, pre_b)
    msgs = T.tn_verdict(kernel, family, dy, x, M, split, kc, part.cpu(), bias.cpu(), stats)
    print(f'[sf_gemm_tn_{kernel}] {family} M={M} N={N} K={K} split={split} kc={kc}: {stats}')
    assert not msgs, '\n'.join(msgs)
    assert torch.equal(G.bits(part0), G.bits(part)), 'part differs between the launch with and the one without bias_part'
    for s, (lo, hi) in enumerate(T.tn_chunks(M, split, kc)):
        if hi == lo:                                                # a chunk entirely past M: exactly zero, written
            assert not part[s].any() and not bias[s].any() and not part0[s].any(), f'empty chunk {s} is not zero'


@pytest.mark.parametrize('family,M,N,K,split,kc', T.TN_SPLITK_CASES, ids=[f'{c[0]}-M{c[1]}-{c[2]}x{c[3]}-s{c[4]}-kc{c[5]}' for c in T.TN_SPLITK_CASES])
def test_tn_splitk_vs_fp64(gpu, family, M, N, K, split, kc):
    """sf_gemm_tn_splitk: 32-token k-tiles per chunk nk in {0, 1, 2, 3, 4, 5, 6, 9, 10} (a prologue shorter than the 4-slot ring, exactly the ring, a wrap, the wait
    ladder 8 / 4 / 0, and chunks entirely past M as train._lin_bwd produces them - exactly zero), valid % 32 in {1, 3, 5, 31} in the last non-empty chunk (partial
    4-row DMA pieces, the per-lane zero-page selection), 1 / 3 / 3 / 9 / 12 tiles (the XCD remap below 8 and off a multiple of 8, tm > 0 and tn > 0; only column tile
    0 writes the bias)."""
    _run_case('splitk', gpu, family, M, N, K, split, kc, {})


@pytest.mark.parametrize('family,M,N,K,split,kc', T.TN_PP_CASES, ids=[f'{c[0]}-M{c[1]}-{c[2]}x{c[3]}-s{c[4]}-kc{c[5]}' for c in T.TN_PP_CASES])
def test_tn_pp_vs_fp64(gpu, family, M, N, K, split, kc):
    """sf_gemm_tn_pp: kc in {128, 256, 384}, a last chunk of 1, 63, 65 and kc - 1 rows (whole 64-row k-tiles past M arrive as zeros from the buffer range check), 1, 4,
    6, 7, 9, 11 and 12 work items (empty XCDs, workgroups that return before any barrier, an uneven last XCD), tm > 0 and tn > 0."""
    _run_case('pp', gpu, family, M, N, K, split, kc, {})


@pytest.mark.parametrize('walk', [0, 1], ids=['two-items', 'three-items'])
def test_tn_pp_item_walk_exact(gpu, walk):
    """N = K = 256, kc = 128 with more chunks than the launch has workgroups (blocks = n_cu & ~7, read from the device): items just above `blocks` - some workgroups
    take two - and above 2 * blocks - some take three: the loader crosses an item boundary twice and the epilogue stores of one item are in flight behind the next
    item's loads.  Integer operands, reference in float64 on the device, bit for bit; three repetitions of the three-item walk must be bit-identical."""
    blocks = max(torch.cuda.get_device_properties(gpu).multi_processor_count & ~7, 8)
    family, M, N, K, split, kc = T.tn_pp_walk_cases(blocks)[walk]
    assert split > (walk + 1) * blocks
    print(f'[sf_gemm_tn_pp walk] {blocks} workgroups, {split} items')
    dy, x = T.tn_operands(family, M, N, K, seed=walk)
    assert T.tn_exact_bound(dy, x, M, kc) < 2 ** 24
    dyd, xd = _upload(dy, x, gpu)
    pre_p = G.canary((split * N * K + TAIL,), torch.float32).to(gpu)
    pre_b = G.canary((split * N + TAIL,), torch.float32).to(gpu)
    part, bias = _launch('pp', dyd, xd, M, N, K, split, kc, True, pre_p, pre_b)
    full = split - 1
    ref = torch.empty(split, N, K, dtype=torch.float32, device=gpu)
    for s0 in range(0, full, 64):                                   # float64 on the device, 64 chunks at a time
        s1 = min(full, s0 + 64)
        a = dyd[s0 * kc:s1 * kc].double().view(s1 - s0, kc, N)
        ref[s0:s1] = (a.transpose(1, 2) @ xd[s0 * kc:s1 * kc].double().view(s1 - s0, kc, K)).float()
    ref[full] = (dyd[full * kc:M].double().t() @ xd[full * kc:M].double()).float()
    bref = torch.stack([dyd[lo:hi].double().sum(0) for lo, hi in T.tn_chunks(M, split, kc)]).float()
    bad = G.bits(part) != G.bits(ref + 0.0)
    assert not bad.any(), f'{int(bad.sum())} elements of part differ bitwise; chunks {bad.any(2).any(1).nonzero().flatten()[:8].tolist()} (workgroups = {blocks})'
    assert torch.equal(G.bits(bias), G.bits(bref + 0.0)), 'bias_part differs bitwise'
    part0, _ = _launch('pp', dyd, xd, M, N, K, split, kc, False, pre_p, pre_b)
    assert torch.equal(G.bits(part0), G.bits(part)), 'part differs between the launch with and the one without bias_part'
    del part0, ref
    if walk == 1:
        for rep in range(3):
            p2, b2 = _launch('pp', dyd, xd, M, N, K, split, kc, True, pre_p, pre_b)
            assert torch.equal(G.bits(p2), G.bits(part)) and torch.equal(G.bits(b2), G.bits(bias)), f'repetition {rep} differs'
            del p2, b2


def _rc(kernel, dyd, ldy, xd, ldx, part, M, N, K, split, kc):
    return _fn(kernel)(dyd.data_ptr(), ldy, xd.data_ptr(), ldx, part.data_ptr(), None, M, N, K, split, kc, _st())


@pytest.mark.parametrize('kernel', ['splitk', 'pp'])
def test_tn_refusals(gpu, kernel):
    """What the argument check does not admit is refused with -1 before any launch: N or K off the tile, kc off its granule, split * kc short of M, a row stride below
    the width (new for sf_gemm_tn_splitk: it used to accept ldy < N and ldx < K) and, for sf_gemm_tn_pp, an empty last chunk and operands whose 32-bit byte offsets
    would wrap (a real small buffer, a large ld).  The same call with valid arguments is accepted."""
    tile, gran = T.TN_TILE[kernel], (64 if kernel == 'splitk' else 128)
    N = K = tile
    kc, M = gran, gran + 5
    dyd = torch.zeros(2 * kc, N, dtype=torch.bfloat16, device=gpu)
    xd = torch.zeros(2 * kc, K, dtype=torch.bfloat16, device=gpu)
    part = torch.full((3, N, K), float('nan'), device=gpu)
    assert _rc(kernel, dyd, N, xd, K, part, M, N, K, 2, kc) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(part[:2]).any() and torch.isnan(part[2]).all()
    part.fill_(float('nan'))
    refused = [
        ('N off the tile', (dyd, N, xd, K, part, M, N - tile // 2, K, 2, kc)),
        ('K off the tile', (dyd, N, xd, K, part, M, N, K + tile // 2, 2, kc)),
        ('kc off its granule', (dyd, N, xd, K, part, M, N, K, 3, kc - gran // 2)),
        ('split * kc < M', (dyd, N, xd, K, part, M, N, K, 1, kc)),
        ('ldy < N', (dyd, N - 8, xd, K, part, M, N, K, 2, kc)),
        ('ldx < K', (dyd, N, xd, K - 8, part, M, N, K, 2, kc)),
        ('ld not a multiple of 8', (dyd, N + 4, xd, K, part, M, N, K, 2, kc)),
    ]
    if kernel == 'pp':
        refused += [
            ('an empty last chunk', (dyd, N, xd, K, part, M, N, K, 3, kc)),
            ('split * kc * ldy * 2 = 2^32', (dyd, 2 ** 32 // (2 * 2 * kc), xd, K, part, M, N, K, 2, kc)),
            ('split * kc * ldx * 2 = 2^32', (dyd, N, xd, 2 ** 32 // (2 * 2 * kc), part, M, N, K, 2, kc)),
        ]
    for what, args in refused:
        assert _rc(kernel, *args) == -1, what
    torch.cuda.synchronize()
    assert torch.isnan(part).all(), 'a refused call wrote'
