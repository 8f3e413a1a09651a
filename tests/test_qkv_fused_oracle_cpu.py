"""No GPU: the oracle of the fused qkv + attention tests (tests/qkv_fused_oracle.py) checked against itself - the reference against explicit loops with torch.softmax in
float64 (both groupings, masked and unmasked, the three record layouts), the two exactness properties of the `exact` generators at every setting used, the condition of
the MXFP8 output test, and the mutation screen: ten wrong variants of a fused kernel, each of which must leave the bars on at least one input family while the unmutated
emulation passes.  The screens run on heads 0 and 1 of one sequence (the reference takes any subset of heads)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qkv_fused_oracle as Q  # noqa: E402

AF, GO = Q.AF, Q.GO
HEADS2 = [0, 1]


def _ops(kind, family, n_seq=1, seed=3, G=Q.N_TOK, **kw):
    if family == 'wide':
        return Q.wide_operands(kind, n_seq, seed, G, **kw)
    return Q.exact_operands(kind, n_seq, family, seed, G, **kw)


_CACHE = {}


def _values(kind, family, which='side', **kw):
    key = (kind, family, which, tuple(sorted(kw.items())))
    if key not in _CACHE:
        ops = _ops(kind, family, **kw)
        _CACHE[key] = (ops,) + Q.qkv_values(ops, which)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the reference against explicit loops
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _loops(qkv, n_seq, G, layout, keep, heads):
    """Explicit loops over sequence, frame or patch, and head; torch.softmax in float64 on keys gathered one by one.  Returns the token rows (n, seq_rows, H, D), the CLS
    row (n, H, D) and the records (m, l, o) per (n, H, P) computed key by key."""
    R = Q.seq_rows(G)
    q, k, v = Q.split_heads(qkv, n_seq, G, heads)
    H = q.shape[2]
    out = torch.zeros(n_seq, R, H, Q.HD, dtype=torch.float64)
    row = torch.zeros(n_seq, H, Q.HD, dtype=torch.float64)
    rows = Q.record_rows(layout, G)
    m = torch.full((n_seq, H, rows.shape[0]), -math.inf, dtype=torch.float64)
    l = torch.zeros(n_seq, H, rows.shape[0], dtype=torch.float64)
    o = torch.zeros(n_seq, H, rows.shape[0], Q.HD, dtype=torch.float64)
    for s in range(n_seq):
        if Q.GROUPING[layout] == 'space':
            groups = [[1 + f * G + t for t in range(G)] for f in range(Q.FRAMES)]
        else:
            groups = [[1 + f * G + p for f in range(Q.FRAMES)] for p in range(G)]
        for h in range(H):
            for toks in groups:
                keys = [r for r in [0] + toks if keep[s, r]]
                sc = Q.SCALE * q[s, toks, h] @ k[s, keys, h].t()
                out[s, toks, h] = torch.softmax(sc, -1) @ v[s, keys, h]
            keys = [r for r in range(R) if keep[s, r]]
            sc = Q.SCALE * k[s, keys, h] @ q[s, 0, h]
            row[s, h] = torch.softmax(sc, 0) @ v[s, keys, h]
            for p in range(rows.shape[0]):
                keys = [r for r in rows[p].tolist() if r >= 0 and keep[s, r]]
                if keys:
                    sc = Q.SCALE * k[s, keys, h] @ q[s, 0, h]
                    m[s, h, p] = sc.max() * Q.LOG2E
                    e = torch.exp(sc - sc.max())
                    l[s, h, p], o[s, h, p] = e.sum(), e @ v[s, keys, h]
    return out, row, (m, l, o)


@pytest.mark.parametrize('layout,G,mask', [('space', 196, None), ('space', 196, 'frame'), ('time2', 196, None), ('time2', 196, 'random20'), ('time2', 196, 'patch'),
                                           ('time', 196, 'random80'), ('time', 36, None), ('time', 4, 'last')])
def test_reference_matches_explicit_loops(layout, G, mask):
    """fused_reference (batched, explicit exponentials, records gathered by record_rows) equals the loops to 1e-12: token rows, the CLS row, every record (m, l, o),
    and the records' float64 merge equals the CLS row and (M, L).  Every row of a sequence is the CLS row or belongs to exactly one group, every key to one record."""
    n = 2
    which = 'side' if layout != 'time' else 'cls'
    ops = Q.exact_operands('bf16', n, 'marked', 11, G, side_differs=True)
    qkv, _ = Q.qkv_values(ops, which)
    keep = Q.key_keep(mask, n, 1, G) if mask else torch.ones(n, Q.seq_rows(G), dtype=torch.bool)
    ref = Q.fused_reference(qkv, n, G, layout, keep, heads=HEADS2)
    want, row, (m, l, o) = _loops(qkv, n, G, layout, keep, HEADS2)
    got = Q.rows_of(ref['tok'].ref, n, G, layout)
    assert (got[:, 1:] - want[:, 1:]).abs().max() <= 1e-12 * want.abs().max()
    assert (ref['row'].ref - row).abs().max() <= 1e-12 * row.abs().max()
    rec = ref['rec']
    assert torch.equal(rec['empty'], l == 0) and rec['m'].shape[-1] == ref['P'] == {'space': 8, 'time2': 33, 'time': G // 4}[layout]
    live = ~rec['empty']
    assert (rec['m'] - m)[live].abs().max() <= 1e-12 * m[live].abs().max().clamp_min(1.0)
    assert (rec['l'] - l).abs().max() <= 1e-12 * l.max() and (rec['o'] - o).abs().max() <= 1e-12 * o.abs().max()
    merged, M, L = Q.merge_records(rec['m'], rec['l'], rec['o'])
    assert (merged - ref['row'].ref).abs().max() <= 1e-12 * row.abs().max()
    assert (M - ref['M']).abs().max() <= 1e-12 * M.abs().max().clamp_min(1.0) and (L - ref['L']).abs().max() <= 1e-12 * L.max()
    count = torch.zeros(Q.seq_rows(G), dtype=torch.int64)
    rows = Q.record_rows(layout, G)
    count.scatter_add_(0, rows[rows >= 0], torch.ones_like(rows[rows >= 0]))
    assert (count == 1).all(), 'every key, the CLS key included, is counted in exactly one record'
    for sec in (ref['tok'], ref['row']):
        assert ((sec.emu - sec.ref).abs() <= sec.bar).all() and (sec.bar > 0).all()


def test_side_index_and_given_rows():
    """The given rows are the host-rounded float64 projection of x_given; with side_differs the X rows at those positions hold other content, and the reference takes
    the given values."""
    ops = Q.exact_operands('bf16', 2, 'marked', 5, side_differs=True)
    idx, side = Q.given_rows(ops, 'side')
    assert idx.numel() == 66 and idx[0] == 0 and idx[1] == 1 + 192 and idx[33] == 1569 and idx[65] == 1569 + 1 + 7 * 196 + 195
    assert not torch.equal(ops['x'][idx], ops['x_given'][idx])
    qkv, _ = Q.qkv_values(ops, 'side')
    assert torch.equal(qkv[idx], side.double())
    from_x, _ = Q.qkv_values(ops, 'side', from_x=True)
    assert (from_x[idx] != qkv[idx]).any(1).all(), 'every given row differs from the projection of its X row'
    other = torch.ones(qkv.shape[0], dtype=torch.bool)
    other[idx] = False
    assert torch.equal(from_x[other], qkv[other])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the exact generators
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['bf16', 'mx'])
@pytest.mark.parametrize('family', Q.EXACT_FAMILIES)
def test_exact_family_is_exact(kind, family):
    """Both exactness properties at every (family, kind) used, with and without bias and with the rows behind the last sequence; MX: the dequantised bytes are the
    values; the stated input statistics: q, k sigma about 0.5 on flat, scores spanning about +-30 on sharp, about -5 on negative, exactly 0 on uniform, and the marks
    in v."""
    for G, bias in ((196, True), (36, False)):
        ops = Q.exact_operands(kind, 1, family, 7, G, bias=bias)
        proj, S = Q.project(ops)
        Q.assert_exact(ops, proj, S)                                                # (qkv_values asserts the same before any use)
        full, Sf = GO.reference(ops['x'], ops['w'], ops['bias'])                     # ... the rows behind the last sequence included
        assert torch.equal(AF._rb(full), full)
        if kind == 'mx':
            assert torch.equal(GO.mx_dequant(ops['xq'], ops['xsc']), ops['x']) and torch.equal(GO.mx_dequant(ops['wq'], ops['wsc']), ops['w'])
            assert (ops['xq'] & 0x7F).max() <= 0x38 and int(ops['xsc'].min()) >= 125 and int(ops['xsc'].max()) <= 127
        else:
            assert ((ops['x'] != 0).sum(1) <= 17).all()
    ops = Q.exact_operands(kind, 1, family, 7)
    qkv, _ = Q.qkv_values(ops, 'side')
    q, k, v = Q.split_heads(qkv, 1, 196)
    s = Q.SCALE * torch.einsum('nqhd,nkhd->nhqk', q[:, 1:197], k[:, :197])
    span = (s.amax(-1) - s.amin(-1)).median().item()
    if family in ('flat', 'marked'):
        assert 0.3 < q.std().item() < 0.9 and 0.3 < k.std().item() < 0.9 and span < 8
    elif family == 'sharp':
        assert span > 40, span                                                      # +-20 at the least for the median query, +-30 for many
    elif family == 'negative':
        assert -6.5 < s.mean().item() < -3.5 and s.max().item() < -2.0
    else:
        assert (s == 0).all()
    if family in ('marked', 'sharp', 'uniform'):
        vt = v[0, 1:].view(8, 196, 12, 64)
        for f, t in ((0, 0), (3, 77), (7, 191), (2, 193)):
            col = 8 + (t + 6 * f) % 48 if t < 192 else 56 + t - 192
            assert (vt[f, t, :, col] >= 1.5).all() and (vt[f, t].abs().amax(0) >= 1.5).sum() == 1
        assert (v[0, 0, :, 60] >= 1.5).all()


@pytest.mark.parametrize('kind', ['bf16', 'mx'])
def test_wide_family_scale(kind):
    ops = Q.wide_operands(kind, 1, 9)
    qkv, dq = Q.qkv_values(ops, 'side')
    q, k, v = Q.split_heads(qkv, 1, 196)
    assert 0.4 < q.pow(2).mean().sqrt().item() < 2.5
    idx = Q.side_index(1)
    assert (dq['full'][idx] == 0).all() and (dq['full'][1:190] > 0).all() and (dq['fp32'] <= dq['full']).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the condition of the MXFP8 output test
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout,family', [('space', 'uniform'), ('time2', 'uniform'), ('time', 'uniform'), ('time', 'marked')])
def test_bf16_output_is_known_bit_for_bit(layout, family):
    """Where the error in front of the bf16 store is below the distance to the next rounding boundary the bf16 output is known bit for bit.  The kernels that pack P to
    bf16 carry u A in that error, which is never below half an ulp of the output: their MXFP8 byte test runs on the `uniform` family (every exponential exactly 1: the
    packing is the identity); sf_qkv_time_attention is fp32 to the store and is known on `marked` as well.  At least 90 % of the elements, and of the 32-blocks."""
    ops, qkv, _ = _values('mx', family, 'side' if layout != 'time' else 'cls')
    ref = Q.fused_reference(qkv, 1, 196, layout, heads=HEADS2)
    sec = ref['tok']
    err = Q.preround_error(sec, packing_exact=family == 'uniform')
    assert Q.known_bf16(sec.ref, err).float().mean().item() >= 0.9
    assert ((sec.emu - sec.ref).abs() <= sec.bar).all()
    flat = lambda x: Q.rows_of(x, 1, 196, layout)[0, 1:].reshape(-1, 128)           # noqa: E731
    _, _, ek, sk = Q.mx_expected(flat(sec.ref), flat(err))
    assert ek.float().mean().item() >= 0.9 and sk.float().mean().item() >= 0.9


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the mutation screen
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _emu_tok(qkv, layout, keep=None, n=1, G=196):
    return Q.fused_reference(qkv, n, G, layout, keep, heads=HEADS2)


def _ratios(ref, mut):
    """Worst ratio of a mutated emulation against the bars of the true reference: token rows, the merged CLS row, the records."""
    r = dict(tok=Q.worst_ratio(mut['tok'].emu, ref['tok']), row=Q.worst_ratio(mut['row'].emu, ref['row']))
    if mut['rec']['m'].shape == ref['rec']['m'].shape:
        part = torch.cat([mut['rec']['m'][..., None], mut['rec']['l'][..., None], mut['rec']['o']], -1)
        part = torch.where(mut['rec']['empty'][..., None], torch.cat([torch.full_like(part[..., :1], -math.inf), torch.zeros_like(part[..., 1:])], -1), part)
        if torch.equal(mut['rec']['empty'], ref['rec']['empty']):
            r['rec'] = max(Q.record_ratios(part, ref['rec']))
        else:
            r['rec'] = float('inf')
    return r


def _roll_patches(x, shift, G=196):
    """Rows (n, R, ..): token (f, p) takes the content of token (f, p + shift)."""
    y = x.clone()
    t = x[:, 1:].reshape(x.shape[0], 8, G, *x.shape[2:])
    y[:, 1:] = torch.roll(t, -shift, 2).reshape(x.shape[0], 8 * G, *x.shape[2:])
    return y


def _mutate(name, family, layout):
    """(reference, mutated run) of one mutation on one family, or None where the mutation does not apply to the layout."""
    which = 'side' if layout != 'time' else 'cls'
    ops, qkv, _ = _values('bf16', family, which, side_differs=(name == 'side_from_x'))
    R = Q.seq_rows()
    ones = torch.ones(1, R, dtype=torch.bool)
    x3 = qkv.view(1, R, 2304)
    if name == 'drop_key_193':
        keep = ones.clone()
        keep[:, 1 + 192::196] = False
        return _emu_tok(qkv, layout), _emu_tok(qkv, layout, keep)
    if name == 'side_of_next_frame':
        y = x3.clone()
        side = x3[:, 1:].view(1, 8, 196, 2304)[:, :, 192:]
        y[:, 1:].view(1, 8, 196, 2304)[:, :, 192:] = torch.roll(side, -1, 1)
        return _emu_tok(qkv, layout), _emu_tok(y.view(R, 2304), layout)
    if name == 'side_flags_ignored':
        return _emu_tok(qkv, layout, Q.key_keep('side', 1)), _emu_tok(qkv, layout, ones)
    if name == 'flag_of_next_row':
        keep = Q.key_keep('random20', 1, 4)
        bad = torch.roll(keep, -1, 1)
        bad[:, 0] = True
        return _emu_tok(qkv, layout, keep), _emu_tok(qkv, layout, bad)
    if name == 'cls_key_in_every_record':
        ref = _emu_tok(qkv, layout)
        rows = Q.record_rows(layout)
        rows = torch.cat([rows, torch.where((rows == 0).any(1, keepdim=True), -1, 0)], 1)   # one more key slot: the CLS row wherever the record lacks it
        q, k, v = Q.split_heads(qkv, 1, 196, HEADS2)
        rec = Q.cls_records(q, k, v, ones, rows, Q.PACKS_P[layout])
        row, _, _ = Q.merge_records(rec['m'], rec['l'], rec['o'])
        mut = dict(tok=ref['tok'], row=AF._Sec(None, None, row, None), rec=rec)
        return ref, mut
    if name == 'heads_swapped':
        ref = _emu_tok(qkv, layout)
        mut = dict(tok=AF._Sec(None, None, ref['tok'].emu[:, :, [1, 0]], None), row=AF._Sec(None, None, ref['row'].emu[:, [1, 0]], None),
                   rec={key: (val[:, [1, 0]] if torch.is_tensor(val) else val) for key, val in ref['rec'].items()})
        return ref, mut
    if name == 'frames_of_next_patch':
        if layout == 'space':
            return None
        y = x3.clone()
        y[:, :, 768:] = _roll_patches(x3[:, :, 768:], 1)                            # k and v of patch p + 1 under the queries of patch p
        return _emu_tok(qkv, layout), _emu_tok(y.view(R, 2304), layout)
    if name == 'zero_slot_leaks':
        keep = Q.key_keep('seam191', 1)
        y = x3.clone()
        y[:, ~keep[0], 768:] = 0.0                                                  # the masked slot holds zeros and is attended with score 0
        return _emu_tok(qkv, layout, keep), _emu_tok(y.view(R, 2304), layout, ones)
    if name == 'side_from_x':
        from_x, _ = Q.qkv_values(ops, which, from_x=True)
        return _emu_tok(qkv, layout), _emu_tok(from_x, layout)
    raise ValueError(name)


MUTATIONS = ['drop_key_193', 'side_of_next_frame', 'side_flags_ignored', 'flag_of_next_row', 'cls_key_in_every_record', 'heads_swapped', 'frames_of_next_patch',
             'zero_slot_leaks', 'side_from_x']


@pytest.mark.parametrize('layout', ['space', 'time2', 'time'])
def test_unmutated_emulation_passes(layout):
    """The emulation of a correct kernel stays inside every bar on every exact family and on wide (with the propagated terms), and inside the statistical limit."""
    which = 'side' if layout != 'time' else 'cls'
    for family in ('marked', 'sharp', 'negative', 'wide'):
        ops, qkv, dq = _values('bf16', family, which)
        emu = Q.emulated_qkv(ops, which) if family == 'wide' else None
        for keep in (None, Q.key_keep('random20', 1, 4)):
            ref = Q.fused_reference(qkv, 1, 196, layout, keep, dq=dq, emu_qkv=emu, heads=HEADS2)
            r = _ratios(ref, dict(tok=ref['tok'], row=ref['row'], rec=ref['rec']))
            assert r['tok'] <= 1.0 and r['row'] <= 1.0 and r['rec'] <= 1e-9, (family, r)
            assert Q.stat_ratio(ref['tok'].emu, ref['tok']) <= 1.0


@pytest.mark.parametrize('name', MUTATIONS)
def test_mutation_is_rejected(name):
    """Each wrong variant leaves the bars of the true reference - on the token rows, the merged CLS row or the records - on at least one of the marked, sharp and negative
    families, for every kernel layout it applies to."""
    for layout in ('space', 'time2', 'time'):
        seen = {}                                                                   # (sf_qkv_time_attention projects tokens 192 .. 195 itself: there the side mutations are plain data / mask errors, and its given row is the CLS row)
        for family in ('marked', 'sharp', 'negative'):
            pair = _mutate(name, family, layout)
            if pair is None:
                break
            r = _ratios(*pair)
            seen[family] = max(r.values())
        if not seen:
            continue
        print(f'{name} on {layout}: worst ratio per family {seen}')
        assert max(seen.values()) > 1.0, f'{name} on {layout}: not detected by any family: {seen}'


def test_mutation_skipped_k_block_is_rejected():
    """Mutation 8 (wide family): one 32-deep k-block of the projection skipped.  The unmutated emulation passes both criteria; the mutated one fails both."""
    ops, qkv, dq = _values('bf16', 'wide', 'side')
    good = Q.emulated_qkv(ops, 'side')
    bad = Q.emulated_qkv(ops, 'side', kblocks=[j for j in range(24) if j != 7])
    for layout in ('space', 'time2'):
        ref = Q.fused_reference(qkv, 1, 196, layout, dq=dq, emu_qkv=good, heads=HEADS2)
        mut = Q.fused_reference(bad, 1, 196, layout, heads=HEADS2)
        assert Q.worst_ratio(ref['tok'].emu, ref['tok']) <= 1.0 and Q.stat_ratio(ref['tok'].emu, ref['tok']) <= 1.0
        e, s = Q.worst_ratio(mut['tok'].emu, ref['tok']), Q.stat_ratio(mut['tok'].emu, ref['tok'])
        print(f'skipped k-block on {layout}: element ratio {e:.3g}, statistical ratio {s:.3g}')
        assert e > 1.0 and s > 1.0
