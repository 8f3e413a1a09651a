"""GPU: the fused "qkv projection + divided attention" launches - sf_qkv_space_attention, sf_qkv_time_attention2 (csrc/sf_qkv_space.hip, sf_qkv_time2.hip on the shared main
loop of sf_qkv_tile.h), sf_qkv_time_attention (sf_qkv_time.hip), their _masked, _mx and MXFP8-output forms, and sf_side_rows - against the float64 oracle of
tests/qkv_fused_oracle.py, computed from the raw operands X, W, bias, side / qkv_cls and key_keep.  No kernel of this library produces an expected value: the given rows
are rounded on the host, the CLS records are merged in float64 here.  Reference, operand families, the derivation of every bar and the criteria: the oracle's docstring;
the oracle itself is screened without a GPU by tests/test_qkv_fused_oracle_cpu.py.  The reference runs on the device in torch float64.

Sizes: the kernels fix 196 tokens x 8 frames, so n_seq sets the size: 1 (48 work items, fewer than workgroups; one row tile per XCD), 3 (an XCD's range of row tiles
crosses a sequence), 6 (288 items on 256 workgroups: the first size at which some workgroups take a second item) and 11 (528 items: two or three per workgroup) on a
256-CU device; sf_qkv_time_attention at n_groups 4, 36 and 196 with 1, 3 and 5 sequences (one ragged 32-patch tile holding three sequences; tiles straddling sequences
with a tail; the product shape).

Every comparison covers all written elements; outputs carry a position-dependent canary that must survive bit for bit in the CLS rows, the pad columns, behind the last
CLS record and, for the MXFP8 form, in the CLS rows' bytes and scale dwords.

Found by this file: sf_qkv_time_attention_mx(_q) at n_groups = 4 with 3 and 5 sequences wrote wrong patch rows (12134 of 73728 and 48376 of 122880 elements outside
the bar, worst err / bar 1.1e4; n_groups 36 and 196 and the bf16 form passed).  Its four shared CLS landing slots hold the two sequences a 32-patch tile may touch,
which holds from n_groups = 28 on; with fewer patches per sequence the waves of a third sequence landed their CLS row in the other tile parity's slot or behind the LDS
allocation.  The launcher now refuses n_groups < 28 with more than two sequences (header comment updated); test_round3_time_attention asserts the refusal for those two
cases.  No output byte of a served shape changed: tests/golden/qkv_fused_digests.json stands.

Measured on an MI355X (73 tests, 16 s; worst error / bar, worst rel-L2 / limit; records o, merged CLS row).  exact: sf_qkv_space_attention 0.61, 0.49 (o 0.59, row 0.19;
masked 0.51, 0.49; _mx 0.57, 0.50), sf_qkv_time_attention2 0.62, 0.50 (o 0.60, row 0.26; masked 0.62, 0.50; _mx 0.61, 0.50), sf_qkv_time_attention 0.66, 0.50 (o 0.007,
row 0.001; masked 0.66, 0.50; _mx 0.66, 0.50) - 0.66 = 1 / 1.5 is an output half a bf16 ulp from the reference: the fp32 kernel sits at the floor of its bar; records
m <= 0.008, l <= 0.005, merged (M, L) <= 0.008.  wide: space 0.10, 0.39 (masked 0.09, 0.40; _mx 0.04, 0.010), time2 0.49, 0.43 (masked 0.61, 0.45; _mx 0.50, 0.017),
time 0.14, 0.43 (masked 0.22, 0.44; _mx 0.09, 0.017): the propagated elementwise bar is loose for the 197-key groups and useful for the 9-key groups, and on MXFP8
operands gemm_oracle.mx_group_term dominates the statistical limit - there the exact family carries the sharp check.  MXFP8 output form: every known byte and scale byte
equal; the share left out as not known (printed under `known share`) is 1.4 % (space), 0 (time2) and 7.1 % (round 3) at the most.  No bar needed an addition after the
measurement; the one change after the first run was the 2^-126 under the m bars (0 / 0 on the `uniform` family, the oracle's docstring)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qkv_fused_oracle as Q  # noqa: E402

AF, GO = Q.AF, Q.GO
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = {'space': 'sf_qkv_space_attention', 'time2': 'sf_qkv_time_attention2', 'time': 'sf_qkv_time_attention'}


def _lib():
    from synchformer_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _err():
    return _lib().sf_last_error().decode(errors='replace')


def _pad_cols(t, ld, fill):
    """(rows, cols) -> (rows, ld) with the pad columns holding `fill` (never read by a correct kernel)."""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


class Case:
    """The operands of one case on the device, in the strides of one launch form.  pad: ldx / ldw a larger multiple of 64 elements (128 bytes), lds_ / ldc / ldo / ldq
    larger multiples of 8."""

    def __init__(self, gpu, kind, family, n_seq, seed=0, G=Q.N_TOK, which='side', side_differs=False, bias=True, pad=False):
        self.gpu, self.kind, self.family, self.n, self.G, self.which, self.pad = gpu, kind, family, n_seq, G, which, pad
        self.key = (kind, family, n_seq, seed, G, which, side_differs, bias)
        if family == 'wide':
            ops = Q.wide_operands(kind, n_seq, seed, G, bias=bias)
        else:
            ops = Q.exact_operands(kind, n_seq, family, seed, G, side_differs=side_differs, bias=bias)
        self.ops = ops
        self.R = Q.seq_rows(G)
        self.rows = n_seq * self.R
        px, pw, p8 = (64, 128, 8) if pad else (0, 0, 0)
        if kind == 'bf16':
            self.ldx, self.ldw = 768 + px, 768 + pw
            self.X = _pad_cols(ops['xb'], self.ldx, 1e4).to(gpu)
            self.W = _pad_cols(ops['wb'], self.ldw, 1e4).to(gpu)
            self.sX = self.sW = None
            self.ldsx = self.ldsw = 0
        else:
            self.ldx, self.ldw = 768 + 2 * px, 768 + pw
            self.X = _pad_cols(ops['xq'], self.ldx, 0x7E).to(gpu)
            self.W = _pad_cols(ops['wq'], self.ldw, 0x7E).to(gpu)
            ra = ((self.rows + 2 + 255) // 256) * 256 + (64 if pad else 0)
            self.sX = GO.mx_planes(ops['xsc'], ra).to(gpu)
            self.sW = GO.mx_planes(ops['wsc'], 2304 + (64 if pad else 0)).to(gpu)
            self.ldsx, self.ldsw = self.sX.stride(0), self.sW.stride(0)
        self.bias = ops['bias'].float().to(gpu) if ops['bias'] is not None else None
        idx, given = Q.given_rows(ops, which)
        self.ldg = 2304 + p8
        self.given = _pad_cols(given, self.ldg, 1e4).to(gpu)
        self.ldo = 768 + p8
        self.rows_alloc = ((self.rows + 255) // 256) * 256
        self._values = None
        self._refs = {}

    def values(self):
        if self._values is None:
            qkv, dq = Q.qkv_values(self.ops, self.which, self.gpu)
            emu = Q.emulated_qkv(self.ops, self.which, self.gpu) if self.family == 'wide' else None
            self._values = (qkv, dq, emu)
        return self._values

    def ref(self, layout, keep=None, mask_name=None):
        key = (layout, mask_name)
        if key not in self._refs:
            qkv, dq, emu = self.values()
            self._refs[key] = Q.fused_reference(qkv, self.n, self.G, layout, keep, dq=dq, emu_qkv=emu)
        return self._refs[key]

    # ---- launches ------------------------------------------------------------------------------------------------------------------------
    def buffers(self, layout, mxq=False, seed=0):
        P = Q.record_rows(layout, self.G).shape[0]
        part_c = GO.canary((self.n * Q.HEADS * P * 66 + 66,), torch.float32)
        b = dict(P=P, part_c=part_c, part=part_c.clone().to(self.gpu))
        if mxq:
            b['q_c'] = GO.canary((self.rows, self.ldo), torch.uint8)
            b['s_c'] = GO.canary((6, self.rows_alloc, 4), torch.uint8)
            b['q'], b['s'] = b['q_c'].clone().to(self.gpu), b['s_c'].clone().to(self.gpu)
        else:
            b['out_c'] = AF._canary(self.rows, self.ldo, seed)
            b['out'] = b['out_c'].clone().to(self.gpu)
        return b

    def launch(self, layout, b, keep=None, n_tok=196, raw=False, **over):
        """One launch of the entry point for (layout, kind, masked, output form) on the buffers `b`; over: replaced arguments for the rejection tests.  Returns rc (raw)
        or raises."""
        L = _lib()
        a = dict(X=_ptr(self.X), ldx=self.ldx, sX=_ptr(self.sX), ldsx=self.ldsx, W=_ptr(self.W), ldw=self.ldw, sW=_ptr(self.sW), ldsw=self.ldsw, bias=_ptr(self.bias),
                 given=_ptr(self.given), ldg=self.ldg, out=_ptr(b.get('out')), ldo=self.ldo, out_q=_ptr(b.get('q')), ldq=self.ldo, out_s=_ptr(b.get('s')),
                 splane=b['s'].stride(0) if 's' in b else 0, part=_ptr(b['part']), n_seq=self.n, last=n_tok if layout != 'time' else self.G, scale=Q.SCALE)
        a.update(over)
        kp = None if keep is None else keep.to(torch.uint8).contiguous().view(-1).to(self.gpu)
        name = NAMES[layout]
        if self.kind == 'bf16':
            args = [a['X'], a['ldx'], a['W'], a['ldw'], a['bias'], a['given'], a['ldg'], a['out'], a['ldo'], a['part'], a['n_seq'], a['last'], a['scale']]
            if kp is not None:
                name += '_masked'
                args.append(_ptr(kp))
        else:
            assert kp is None
            args = [a['X'], a['ldx'], a['sX'], a['ldsx'], a['W'], a['ldw'], a['sW'], a['ldsw'], a['bias'], a['given'], a['ldg']]
            if layout == 'time':
                name += '_mx_q' if a['out_q'] is not None or over.get('force_q') else '_mx'
                args += [a['out_q'], a['ldq'], a['out_s'], a['splane']] if name.endswith('_q') else [a['out'], a['ldo']]
            else:
                name += '_mx'
                args += [a['out'], a['ldo'] if a['out'] is not None else 0, a['out_q'], a['ldq'] if a['out_q'] is not None else 0, a['out_s'], a['splane']]
            args += [a['part'], a['n_seq'], a['last'], a['scale']]
        rc = getattr(L, name)(*args, _st())
        self.last_name = name
        if raw:
            return rc
        from synchformer_amd import _lib as LL
        LL.check(rc, name)
        return rc

    # ---- checks --------------------------------------------------------------------------------------------------------------------------
    def label(self, layout, masked=False, form=''):
        return f"{NAMES[layout]}{'_masked' if masked else ''}{'_mx' if self.kind == 'mx' else ''}{form} [{'exact' if self.family != 'wide' else 'wide'}]"

    def check(self, layout, b, ref, masked=False):
        """Token rows, canaries, records, the float64 merge of the kernel's records against the reference's CLS row and (M, L)."""
        torch.cuda.synchronize()
        name = self.label(layout, masked)
        out = b['out']
        got = Q.tokens_of(out.double(), self.n, self.G, layout)
        assert torch.isfinite(got).all(), f'{name}: non-finite output'
        AF._check_section(name, 'token rows', got, ref['tok'])
        written = torch.zeros(self.n, self.R, self.ldo, dtype=torch.bool)
        written[:, 1:, :768] = True
        AF._assert_untouched(out.cpu(), b['out_c'], written.view(self.rows, self.ldo), name)
        self.check_records(name, b, ref)

    def check_records(self, name, b, ref):
        P = b['P']
        raw = b['part'].cpu()
        nrec = self.n * Q.HEADS * P * 66
        assert torch.equal(raw[nrec:].view(torch.int32), b['part_c'][nrec:].view(torch.int32)), f'{name}: floats behind the last CLS record were written'
        part = raw[:nrec].double().view(self.n, Q.HEADS, P, 66).to(self.gpu)
        empty = ref['rec']['empty']
        assert (part[..., 0][empty] == -math.inf).all(), f'{name}: the record of a group without a kept key must hold m = -inf'
        AF._check_records(name, part, ref['rec'])
        row, M, L = Q.merge_records(part[..., 0], part[..., 1], part[..., 2:])
        assert torch.isfinite(row).all(), f'{name}: the records do not merge cleanly'
        AF._check_section(name + ' merged CLS row', 'CLS row', row, ref['row'])
        AF._check_stats(name + ' merged', torch.stack([M, L], -1), ref)


_CASES = {}


def _case(gpu, *a, **kw):
    """Cases are shared among the tests that need them (operands and references are computed once and left unchanged); a handful are kept."""
    key = (a, tuple(sorted(kw.items())))
    if key not in _CASES:
        while len(_CASES) >= 6:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = Case(gpu, *a, **kw)
    return _CASES[key]


def _run(case, layout, keep=None, mask_name=None):
    b = case.buffers(layout)
    case.launch(layout, b, keep)
    case.check(layout, b, case.ref(layout, keep, mask_name), masked=keep is not None)
    return b


# ======================================================================================================================================
# 1. sf_qkv_space_attention, sf_qkv_time_attention2: bf16 and _mx to bf16
# ======================================================================================================================================
VARIANTS = {'flat': dict(), 'marked': dict(pad=True, side_differs=True), 'sharp': dict(bias=False), 'negative': dict(), 'uniform': dict(pad=True)}


@pytest.mark.gpu
@pytest.mark.parametrize('n_seq', [1, 3])
@pytest.mark.parametrize('kind', ['bf16', 'mx'])
@pytest.mark.parametrize('layout', ['space', 'time2'])
def test_fused_exact_families(gpu, layout, kind, n_seq):
    """exact x {flat, marked, sharp, negative}: the projection is exact, the kernel is held to the attention bars of the arithmetic its epilogue copies (attn_mfma_kernel:
    P packed to bf16).  marked runs on padded strides with `side` differing from the projection of the X rows it stands for; sharp runs without bias."""
    for i, family in enumerate(('flat', 'marked', 'sharp', 'negative')):
        _run(_case(gpu, kind, family, n_seq, seed=10 + i, **VARIANTS[family]), layout)


@pytest.mark.gpu
@pytest.mark.parametrize('n_seq', [6, 11])
@pytest.mark.parametrize('kind', ['bf16', 'mx'])
@pytest.mark.parametrize('layout', ['space', 'time2'])
def test_fused_tile_walk(gpu, layout, kind, n_seq):
    """Several work items per workgroup (operands re-landed behind the epilogue barrier, the tcount unit rotating): exact-marked on padded strides, and wide under the
    elementwise bar with the propagated projection error and the statistical criterion."""
    _run(_case(gpu, kind, 'marked', n_seq, seed=20, pad=True), layout)
    _run(_case(gpu, kind, 'wide', n_seq, seed=21, bias=(n_seq == 6)), layout)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['bf16', 'mx'])
def test_fused_wide_small(gpu, kind):
    """wide at n_seq 1 and 3 as well (with bias, padded at 3)."""
    for n_seq in (1, 3):
        case = _case(gpu, kind, 'wide', n_seq, seed=22, pad=(n_seq == 3))
        for layout in ('space', 'time2'):
            _run(case, layout)


# ======================================================================================================================================
# 2. masked forms
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('pattern', Q.MASKS)
@pytest.mark.parametrize('layout', ['space', 'time2', 'time'])
def test_masked_forms(gpu, layout, pattern):
    """_masked of the three bf16 kernels against the float64 reference with the same flags, on exact-marked and wide: 20 % / 80 % dropped at random, one whole frame (a
    space record with m = -inf, l = 0 that merges cleanly), one patch in all 8 frames (a time group whose only key is the CLS key), the side tokens only, token 191 or
    192 (the seam between projected and side tokens), the last token of the last sequence; all ones is bit-identical to the unmasked launch.  The CLS flag is 1."""
    n = 2
    which = 'side' if layout != 'time' else 'cls'
    keep = Q.key_keep(pattern, n, 3)
    for family, seed in (('marked', 30), ('wide', 31)):
        case = _case(gpu, 'bf16', family, n, seed=seed, which=which)
        b = _run(case, layout, keep, pattern)
        if pattern == 'ones':
            u = case.buffers(layout)
            case.launch(layout, u)
            torch.cuda.synchronize()
            assert torch.equal(b['out'].view(torch.int16), u['out'].view(torch.int16)) and torch.equal(b['part'].view(torch.int32), u['part'].view(torch.int32)), \
                'an all-ones mask must be bit-identical to the unmasked launch'


# ======================================================================================================================================
# 3. sf_qkv_time_attention (round 3), _mx
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('n_seq', [1, 3, 5])
@pytest.mark.parametrize('G', [4, 36, 196])
@pytest.mark.parametrize('kind', ['bf16', 'mx'])
def test_round3_time_attention(gpu, kind, G, n_seq):
    """sf_qkv_time_attention away from n_groups = 196: its 32-patch tiles straddle sequences.  fp32 to the store (attn_tiny64_kernel: A = 0).  bf16: both schedules of
    sf_qkv_time_force_schedule pass the oracle and are bit-identical to each other on the exact family."""
    L = _lib()
    for family, seed, kw in (('marked', 40, dict(pad=True, side_differs=True)), ('negative', 41, dict(bias=True)), ('wide', 42, dict())):
        case = _case(gpu, kind, family, n_seq, seed=seed, G=G, which='cls', **kw)
        if kind == 'mx' and G < 28 and n_seq > 2:                                  # refused: see the module docstring (found by this test)
            for mxq in (False, True):
                b = case.buffers('time', mxq=mxq)
                _refused(case, 'time', b, 'n_groups < 28 with more than two sequences')
                assert 'n_groups < 28' in _err()
            continue
        if kind == 'mx':
            if family == 'marked':
                _check_mxq(case, 'time', False)                                    # _mx and _mx_q: fp32 to the store, the bf16 output is known on this family
            else:
                _run(case, 'time')
            continue
        outs = []
        try:
            for sched in (0, 1):
                L.sf_qkv_time_force_schedule(sched)
                outs.append(_run(case, 'time'))
        finally:
            L.sf_qkv_time_force_schedule(-1)
        if family != 'wide':
            assert torch.equal(outs[0]['out'].view(torch.int16), outs[1]['out'].view(torch.int16)), 'the two schedules differ on exact operands'
            assert torch.equal(outs[0]['part'].view(torch.int32), outs[1]['part'].view(torch.int32)), 'the two schedules differ in the CLS records on exact operands'


# ======================================================================================================================================
# 4. sf_side_rows
# ======================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('n_seq', [1, 3])
def test_side_rows(gpu, n_seq):
    """bf16 rows and e4m3 rows with their 6 scale planes against index_select on the host-side index, on padded byte strides; every byte outside the written rows and
    scale dwords keeps its canary."""
    L = _lib()
    rows = n_seq * 1569
    idx = Q.side_index(n_seq)
    g = GO.gen(50 + n_seq)
    for row_bytes, planes in ((1536, 0), (768, 6)):
        ldx, ldo = row_bytes + 128, row_bytes + 64
        X = torch.randint(0, 256, (rows, ldx), generator=g, dtype=torch.uint8)
        can = GO.canary((n_seq * 33 + 2, ldo), torch.uint8)
        out = can.clone().to(gpu)
        ra, rs = ((rows + 255) // 256) * 256, 64 * ((n_seq * 33 + 63) // 64) + 64
        sX = torch.randint(0, 256, (6, ra, 4), generator=g, dtype=torch.uint8)
        scan = GO.canary((6, rs, 4), torch.uint8)
        sOut = scan.clone().to(gpu)
        Xd, sXd = X.to(gpu), sX.to(gpu)
        rc = L.sf_side_rows(_ptr(Xd), ldx, _ptr(out), ldo, row_bytes, _ptr(sXd) if planes else None, sXd.stride(0) if planes else 0, _ptr(sOut) if planes else None,
                            sOut.stride(0) if planes else 0, planes, n_seq, 196, _st())
        assert rc == 0, _err()
        torch.cuda.synchronize()
        want = can.clone()
        want[:n_seq * 33, :row_bytes] = X.index_select(0, idx)[:, :row_bytes]
        assert torch.equal(out.cpu(), want), f'sf_side_rows ({row_bytes} bytes per row): rows differ from index_select, or bytes outside them were written'
        swant = scan.clone()
        if planes:
            swant[:, :n_seq * 33] = sX.index_select(1, idx)
        assert torch.equal(sOut.cpu(), swant), 'sf_side_rows: scale dwords differ from index_select, or dwords outside them were written'


# ======================================================================================================================================
# 5. argument edges
# ======================================================================================================================================
def _intact(case, b):
    torch.cuda.synchronize()
    for dev, can in (('out', 'out_c'), ('q', 'q_c'), ('s', 's_c'), ('part', 'part_c')):
        if dev in b:
            assert torch.equal(GO.bits(b[dev].cpu()), GO.bits(b[can])), f'{case.last_name}: a refused launch wrote to {dev}'


def _refused(case, layout, b, what, **over):
    rc = case.launch(layout, b, raw=True, **over)
    assert rc == -1, f'{what}: expected -1, got {rc}'
    assert NAMES[layout] in _err(), f'{what}: sf_last_error does not name the entry point: {_err()!r}'
    _intact(case, b)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['space', 'time2'])
def test_argument_edges_tile_kernels(gpu, layout):
    """The rules of qkt_check_args that no other file asks for: each refused launch returns -1, names its entry point and writes nothing; n_seq = 0 returns 0 and
    writes nothing."""
    case = _case(gpu, 'bf16', 'flat', 1, seed=10)
    b = case.buffers(layout)
    _refused(case, layout, b, 'n_tok != 196', n_tok=195)
    _refused(case, layout, b, 'ldx not a multiple of 64 elements', ldx=776)
    _refused(case, layout, b, 'ldw not a multiple of 64 elements', ldw=800)
    _refused(case, layout, b, 'out aliasing X', out=_ptr(case.X))
    _refused(case, layout, b, 'misaligned X', X=_ptr(case.X) + 2)
    _refused(case, layout, b, 'misaligned out', out=_ptr(b['out']) + 2)
    _refused(case, layout, b, 'ldo not a multiple of 8', ldo=772)
    assert case.launch(layout, b, raw=True, n_seq=0) == 0
    _intact(case, b)
    mx = _case(gpu, 'mx', 'flat', 1, seed=10)
    bo, bq = mx.buffers(layout), mx.buffers(layout, mxq=True)
    _refused(mx, layout, bo, 'ldx not a multiple of 128 bytes', ldx=832)
    both = dict(bo, q=bq['q'], s=bq['s'], q_c=bq['q_c'], s_c=bq['s_c'])
    _refused(mx, layout, both, 'both out and out_q')
    _refused(mx, layout, bo, 'neither out nor out_q', out=None)
    _refused(mx, layout, bq, 'out_q aliasing X', out_q=_ptr(mx.X))
    _refused(mx, layout, bq, 'splane too small', splane=mx.rows * 4 - 4)
    _refused(mx, layout, bq, 'out_q without out_s', out_s=None)
    _refused(mx, layout, bo, 'misaligned sX', sX=_ptr(mx.sX) + 4)
    assert mx.launch(layout, bq, raw=True, n_seq=0) == 0
    _intact(mx, bq)


@pytest.mark.gpu
def test_argument_edges_round3(gpu):
    """qkv_time_impl / qkv_time_mx_impl: n_groups % 4 != 0, a misaligned operand, a stride that is no multiple of 8, out_q aliasing X, splane too small."""
    case = _case(gpu, 'bf16', 'flat', 1, seed=43, G=36, which='cls')
    b = case.buffers('time')
    _refused(case, 'time', b, 'n_groups % 4 != 0', last=34)
    _refused(case, 'time', b, 'misaligned W', W=_ptr(case.W) + 2)
    _refused(case, 'time', b, 'ldo not a multiple of 8', ldo=772)
    assert case.launch('time', b, raw=True, n_seq=0) == 0
    _intact(case, b)
    mx = _case(gpu, 'mx', 'flat', 1, seed=43, G=36, which='cls')
    bo, bq = mx.buffers('time'), mx.buffers('time', mxq=True)
    _refused(mx, 'time', bo, 'n_groups % 4 != 0 (MX)', last=34)
    _refused(mx, 'time', bq, 'out_q aliasing X', out_q=_ptr(mx.X))
    _refused(mx, 'time', bq, 'splane too small', splane=mx.rows * 4 - 4)
    _refused(mx, 'time', bo, 'misaligned qkv_cls', given=_ptr(mx.given) + 2)
    assert mx.launch('time', bq, raw=True, n_seq=0) == 0
    _intact(mx, bq)


# ======================================================================================================================================
# 6. MXFP8 output form
# ======================================================================================================================================
def _unplane(s, rows):
    return s[:, :rows].permute(1, 0, 2).reshape(rows, 24)


def _check_mxq(case, layout, family_exact_packing):
    """out_q / out_s of one _mx kernel: the host quantisation of the reference's bf16 output wherever that is known bit for bit (>= 90 % of the elements and of the scale
    bytes), the host quantisation of the kernel's own bf16 output everywhere, the canaries, the records bit-identical to the bf16 form's."""
    name = case.label(layout, form=' to MXFP8')
    ref = case.ref(layout)
    bo, bq = case.buffers(layout), case.buffers(layout, mxq=True)
    case.launch(layout, bo)
    case.launch(layout, bq)
    case.check(layout, bo, ref)
    torch.cuda.synchronize()
    q, s = bq['q'].cpu(), bq['s'].cpu()
    patch = torch.ones(case.n, case.R, dtype=torch.bool)
    patch[:, 0] = False
    patch = patch.view(-1)
    wq = torch.zeros(case.rows, case.ldo, dtype=torch.bool)
    wq[patch, :768] = True
    assert GO.canary_damage(q, bq['q_c'], wq) is None, f'{name}: bytes of the CLS rows or of the pad columns were written'
    ws = torch.zeros(6, case.rows_alloc, 4, dtype=torch.bool)
    ws[:, :case.rows][:, patch] = True
    assert GO.canary_damage(s, bq['s_c'], ws) is None, f'{name}: scale dwords of the CLS rows or behind the last row were written'
    assert torch.equal(bq['part'].view(torch.int32), bo['part'].view(torch.int32)), f'{name}: the CLS records differ from the bf16 form\'s'
    own_q, own_s = GO.mx_quant_ref(bo['out'].cpu()[:, :768].contiguous())
    got_q, got_s = q[:, :768], _unplane(s, case.rows)
    assert torch.equal(got_q[patch], own_q[patch]) and torch.equal(got_s[patch], own_s[patch]), f'{name}: not the MX quantisation of the bf16 form\'s output'
    sec = ref['tok']
    flat = lambda x: Q.rows_of(x, case.n, case.G, layout).reshape(case.rows, 768)      # noqa: E731
    exp_q, exp_s, ek, sk = Q.mx_expected(flat(sec.ref), flat(Q.preround_error(sec, packing_exact=family_exact_packing)))
    fe, fs = ek[patch].float().mean().item(), sk[patch].float().mean().item()
    assert fe >= 0.9 and fs >= 0.9, f'{name}: only {fe:.3f} of the bytes / {fs:.3f} of the scales are known bit for bit: the input does not serve'
    bad_q, bad_s = (got_q != exp_q) & ek & patch[:, None], (got_s != exp_s) & sk & patch[:, None]
    assert not bad_q.any() and not bad_s.any(), f'{name}: {int(bad_q.sum())} bytes and {int(bad_s.sum())} scale bytes differ from the quantised reference'
    AF._worst(name + ' known share', 1.0 - fe)


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['space', 'time2', 'time'])
def test_mxfp8_output_form(gpu, layout):
    """`uniform` (every exponential exactly 1: no packing error, the bf16 output known bit for bit) for the three kernels, and `marked` for sf_qkv_time_attention_mx_q,
    which is fp32 to its store.  n_seq = 3, padded ldq."""
    which = 'side' if layout != 'time' else 'cls'
    _check_mxq(_case(gpu, 'mx', 'uniform', 3, seed=60, which=which, pad=True), layout, True)
    if layout == 'time':
        _check_mxq(_case(gpu, 'mx', 'marked', 3, seed=61, which=which), layout, False)


# ======================================================================================================================================
# 7. SF_QS_PAIR_CHUNK / SF_QT2_PAIR_CHUNK
# ======================================================================================================================================
def _pair_chunk_digests(gpu):
    """SHA-256 of the output bytes and of cls_partial of both tile kernels on one exact and one wide case at n_seq = 6."""
    out = {}
    for family, seed in (('marked', 70), ('wide', 71)):
        case = Case(gpu, 'bf16', family, 6, seed=seed)
        for layout in ('space', 'time2'):
            b = case.buffers(layout)
            case.launch(layout, b)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            h.update(b['out'].cpu().view(torch.int16).numpy().tobytes())
            h.update(b['part'].cpu().numpy().tobytes())
            out[f'{family}/{layout}'] = h.hexdigest()
    return out


@pytest.mark.gpu
def test_pair_chunk_is_bit_identical(gpu):
    """The head pairs per sweep only reorder the work items: a non-default divisor of 6 (read once per process, hence one fresh child process) gives the same bytes."""
    want = _pair_chunk_digests(gpu)
    env = dict(os.environ, SF_QS_PAIR_CHUNK='2', SF_QT2_PAIR_CHUNK='3')
    code = (f'import sys, json, torch; sys.path.insert(0, {HERE!r}); sys.path.insert(0, {os.path.dirname(HERE)!r}); import test_qkv_fused_gpu as T; '
            'print("DIGESTS " + json.dumps(T._pair_chunk_digests(torch.device("cuda:0"))))')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('DIGESTS ')]
    assert line, r.stdout[-2000:]
    assert json.loads(line[-1][8:]) == want


# ======================================================================================================================================
# 8. report
# ======================================================================================================================================
@pytest.mark.gpu
def test_zz_report_worst_ratios(gpu):
    """Worst error / bar and rel-L2 / limit per kernel and form over this module's runs."""
    mine = {k: v for k, v in AF.WORST.items() if k.startswith('sf_qkv')}
    assert mine, 'no comparison ran'
    for k in sorted(mine):
        print(f'worst ratio {k}: {mine[k]:.3g}')
