"""CPU: the harness of tests/test_gemm_gpu.py would reject a subtly wrong kernel.  The fp32 emulation of tests/gemm_oracle.py stands in for a kernel's output:
as it is, it must pass both criteria of both operand families for every epilogue; corrupted on ONE 64 x 64 block of a 300 x 320 x 256 product in each of
seven ways, it must be rejected - by inequality of bits in the `exact` family, by at least one of the two criteria in the `wide` family.  The float64 reference
itself is checked against three explicit Python loops.  The MXFP8 kernels' wider bar (see gemm_oracle.mx_group_term) goes through the same corruptions; what it
cannot reject is listed at MX_WIDE_BLIND.

The last corruption - the output rounded toward zero instead of to nearest-even - exists for the bf16 outputs only: an fp32 output is not rounded separately
(its rounding is the last addition's), and in the `exact` family an fp32 result is an integer below 2^24, which every rounding mode leaves alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as G  # noqa: E402

M, N, K = 300, 320, 256
R0, C0 = 128, 192                       # the corrupted block: rows 128..191, columns 192..255
D16 = G.depth(K, '16x16x32')
EPILOGUES = [(obf, gelu, res) for obf in (False, True) for gelu in (False, True) for res in (False, True)]
EPI_IDS = [f'{"bf16" if o else "f32"}{"-gelu" if g else ""}{"-res" if r else ""}' for o, g, r in EPILOGUES]
CORRUPTIONS = ['kblock_dropped', 'kblock_twice', 'row_groups_swapped', 'acc_rounded_bf16', 'bias_of_next_column', 'residual_of_wrong_row', 'output_rtz']

_cache = {}


def _case(family):
    if family not in _cache:
        if family.startswith('mx-'):
            op = G.mx_operands(family[3:], M, N, K, seed=13 if family == 'mx-exact' else 14)
        else:
            op = G.operands(family, M, N, K, seed=11 if family == 'exact' else 12, a_rows=M)
        pre, S = G.reference(op['a'], op['w'], op['bias'])
        _cache[family] = (op, pre, S)
    return _cache[family]


def _good(family, obf, gelu, res):
    key = (family, obf, gelu, res)
    if key not in _cache:
        op, pre, S = _case(family)
        r = op['res'] if res else None
        if family.startswith('mx-'):                   # the MXFP8 kernels' bar: d of the 64-deep scaled MFMA + the instruction's group truncation
            extra = G.mx_group_term(op['a'], op['w']) if family == 'mx-wide' else None
            exp = G.expected(pre, S, r, gelu=gelu, out_bf16=obf, d=G.depth(K, '32x32x64'), exact_pre=family == 'mx-exact', extra=extra)
        else:
            exp = G.expected(pre, S, r, gelu=gelu, out_bf16=obf, d=D16, exact_pre=family == 'exact')
        emu = G.emulate(op['a'], op['w'], op['bias'], r, gelu=gelu, out_bf16=obf)
        _cache[key] = (exp, emu)
    return _cache[key]


def _corrupt(family, obf, gelu, res, how):
    """The emulation with one 64 x 64 block replaced by what a kernel with defect `how` would have written there."""
    op, _, _ = _case(family)
    _, emu = _good(family, obf, gelu, res)
    rs, cs = slice(R0, R0 + 64), slice(C0, C0 + 64)
    a, w, bias, r = op['a'][rs], op['w'][cs], op['bias'][cs], (op['res'][rs, cs] if res else None)
    kw = dict(gelu=gelu, out_bf16=obf)
    nkb = K // 32
    if how == 'kblock_dropped':
        blk = G.emulate(a, w, bias, r, kblocks=[j for j in range(nkb) if j != 5], **kw)
    elif how == 'kblock_twice':
        blk = G.emulate(a, w, bias, r, kblocks=[0, 1, 2, 3, 3, 4, 5, 6, 7], **kw)
    elif how == 'row_groups_swapped':
        blk = emu[rs, cs].clone()
        blk[16:32], blk[32:48] = emu[rs, cs][32:48], emu[rs, cs][16:32]
    elif how == 'acc_rounded_bf16':
        blk = G.emulate(a, w, bias, r, round_acc_after=nkb // 2, **kw)
    elif how == 'bias_of_next_column':
        blk = G.emulate(a, w, op['bias'][C0 + 1:C0 + 65], r, **kw)
    elif how == 'residual_of_wrong_row':
        blk = G.emulate(a, w, bias, op['res'][R0 + 1:R0 + 65, cs], **kw)
    elif how == 'output_rtz':
        blk = G.emulate(a, w, bias, r, rtz=True, **kw)
    else:
        raise ValueError(how)
    out = emu.clone()
    out[rs, cs] = blk
    return out


def test_reference_against_python_loops():
    """reference() on a 5 x 7 x 64 case against three explicit loops in float64 (Python floats), S included."""
    op = G.operands('wide', 5, 7, 64, seed=3, a_rows=5)
    pre, S = G.reference(op['a'], op['w'], op['bias'])
    a, w, b = op['a'].double().tolist(), op['w'].double().tolist(), op['bias'].double().tolist()
    for m in range(5):
        for n in range(7):
            acc, s = 0.0, 0.0
            for k in range(64):
                acc += a[m][k] * w[n][k]
                s += abs(a[m][k] * w[n][k])
            acc, s = acc + b[n], s + abs(b[n])
            assert abs(pre[m, n].item() - acc) <= 1e-13 * s and abs(S[m, n].item() - s) <= 1e-13 * s, (m, n)
    exp = G.expected(pre, S, op['res'], gelu=False, out_bf16=False, d=D16)
    assert torch.equal(exp['ref'], pre + op['res'].double())
    # the integer family is an integer computation: float64 == int64, and fp32 holds it exactly
    ope = G.operands('exact', 5, 7, 64, seed=4, a_rows=5)
    pre_e, _ = G.reference(ope['a'], ope['w'], ope['bias'])
    ref_i = ope['a'].long() @ ope['w'].long().t() + ope['bias'].long()
    assert torch.equal(pre_e, ref_i.double()) and torch.equal(pre_e.float().double(), pre_e)


@pytest.mark.parametrize('obf,gelu,res', EPILOGUES, ids=EPI_IDS)
@pytest.mark.parametrize('family', ['exact', 'wide', 'mx-exact', 'mx-wide'])
def test_uncorrupted_emulation_passes(family, obf, gelu, res):
    exp, emu = _good(family, obf, gelu, res)
    if family.endswith('exact') and not gelu:
        assert G.exact_mismatch(emu, exp['ref'], obf) is None
    r = G.wide_check(emu, exp, emu)
    assert r['msg'] is None, r['msg']
    assert r['stat'] <= 1.0 / G.STAT_FACTOR + 1e-12          # the emulation measured with its own yardstick


# every corruption on every epilogue it can occur in: a wrong residual row needs a residual, a wrong output rounding a bf16 output (module docstring)
CORRUPT_CASES = [(f, e, how) for f in ('exact', 'wide') for e in EPILOGUES for how in CORRUPTIONS
                 if not (how == 'residual_of_wrong_row' and not e[2]) and not (how == 'output_rtz' and not e[0])]
# The same corruptions under the MXFP8 kernels' bar (d of the 64-deep scaled MFMA + gemm_oracle.mx_group_term, operands of gemm_oracle.mx_operands).  The integer
# family rejects every one of them by bits.  The wide family rejects every one but the two ROUNDING corruptions on a bf16 output: the matrix instruction's own
# truncation (up to 2^-13 of a group's largest product per product; measured on the device at 0.4 of that bound) is of the size of a bf16 rounding
# of a partial sum for these operands, so no bar that admits the instruction can refuse them - measured here: accumulator rounded to bf16 mid-loop, worst
# err / bar 0.76 - 0.92 on the four bf16 epilogues; output rounded toward zero 0.99 / 0.86 on bf16 and bf16 + GELU (rejected with a residual).  For the MXFP8
# kernels a wrong rounding is therefore caught by the integer family alone.
MX_WIDE_BLIND = {((True, g, r), 'acc_rounded_bf16') for g in (False, True) for r in (False, True)} | {((True, g, False), 'output_rtz') for g in (False, True)}
CORRUPT_CASES += [(f, e, how) for f in ('mx-exact', 'mx-wide') for e in EPILOGUES for how in CORRUPTIONS
                  if not (how == 'residual_of_wrong_row' and not e[2]) and not (how == 'output_rtz' and not e[0])
                  and not (f == 'mx-wide' and (e, how) in MX_WIDE_BLIND)]


@pytest.mark.parametrize('family,epi,how', CORRUPT_CASES, ids=[f'{f}-{EPI_IDS[EPILOGUES.index(e)]}-{h}' for f, e, h in CORRUPT_CASES])
def test_corruption_is_rejected(family, epi, how):
    obf, gelu, res = epi
    exp, emu = _good(family, obf, gelu, res)
    bad = _corrupt(family, obf, gelu, res, how)
    assert not torch.equal(G.bits(bad), G.bits(emu)), 'the corruption changed nothing'
    outside = torch.ones(M, N, dtype=torch.bool)
    outside[R0:R0 + 64, C0:C0 + 64] = False
    assert torch.equal(G.bits(bad)[outside], G.bits(emu)[outside])
    if family.endswith('exact') and not gelu:
        msg = G.exact_mismatch(bad, exp['ref'], obf)
        assert msg is not None
    else:
        r = G.wide_check(bad, exp, emu)
        assert r['msg'] is not None and (r['elem'] > 1.0 or r['stat'] > 1.0), (r['elem'], r['stat'])
