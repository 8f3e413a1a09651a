"""CPU screen of tests/tower_bwd_oracle.py (no GPU): is the oracle right, do the criteria pass another draw of the same roundings, and do they reject every plant?

Configurations (models cached per module): visual A = 1 segment, 1 block; visual B = 2 segments, 1 block with DropPath vectors given by hand (space: segment 1
dropped, MLP: segment 0 dropped, kept scale 1 / 0.7) for the plants that need a second segment; audio = 2 segments, 1 AST layer.  None of the plants needs a
neighbouring block.  The "engine" of the screen is the stepped model evaluated in float32.

Figures of this screen (printed by every test; ratios are err / bar, a pass is <= 1):
  split forward = oracle.synchformer_cpu's: 0.0 (visual, with DropPath vectors), 0.0 (audio).
  stepped(rnd=False) vs exact, worst relative deviation over out, every G_b, every gradient: A 2.0e-15, B 1.9e-15, audio 1.9e-15 (bar 1e-10).
  exact vs fp32 autograd: visual B worst 9.5e-07 (patch_embed_3d.proj.weight), median 3.6e-07; audio worst 9.7e-07, median 1.6e-07 (bar 1e-4).
  the float32 draw, (A) row / sum / mean per class, stepped noise (rel-RMS of G_b) in brackets:
    A time   cls 0.64 0.64 0.64 [5.2e-3]  side 0.72 0.68 0.68 [6.9e-3]  patch 0.75 0.66 0.66 [6.8e-3]
    A space  cls 0.67 0.67 0.67 [5.0e-3]  side 0.70 0.66 0.66 [5.2e-3]  patch 0.75 0.66 0.66 [5.2e-3]
    A mlp    cls 0 (exactly zero in all three: the final norm drops the CLS rows)  side 0.72 0.66 0.64 [6.5e-3]  patch 0.81 0.66 0.65 [6.3e-3]
    B        kept classes 0.66 - 0.80 (worst: mlp patch_kept row 0.80), dropped classes exactly 0 in all three models
    audio    attn cls 0.67 0.66 0.66 [5.4e-3] patch 0.68 0.64 0.64 [5.5e-3]; mlp patch 0.73 0.66 0.65 [6.2e-3]
    (G) worst tensor / worst block: A 0.68 (agg norm2.bias) / 0.77 (agg out_proj.weight); B 0.69 / 0.85 (blocks.0.mlp.fc2.weight); audio 0.70 / 0.74
    An engine whose error equals the stepped model's own sits at 0.67.
  plants (what exceeded its bar; all eight caught by the criteria as first stated, none had to be sharpened):
    dp_wrong_site              (A) row / sum / mean of space 112 - 146 in the kept classes, inf in the dropped ones (a dropped branch must add exactly 0); time 68 - 143;
                               (G) attn.qkv / attn.proj weights and biases 157 - 173
    bias_unscaled              (G) tensor blocks.0.mlp.fc2.bias 213
    stale_branch_head          (A) space 70 - 86, time 28 - 46; (G) attn.qkv / attn.proj 75 - 86
    cls_kv_group_missing       (A) row / sum / mean of the space CLS row 49; (G) attn.qkv.weight tensor 2.0, block 3.9
    cls_kv_group_missing_time  one partial of 196: (G) block of timeattn.qkv.weight 2.58; (A) row / sum / mean of the time CLS row 1.02; (G) tensor cls_token 1.02
    cls_dq_first_group_only    (G) block of timeattn.qkv.weight 6.8 (only the per-block criterion: the CLS query's dq is one row of 1 569).  Planted in the time branch:
                               in the last block's space branch the CLS query's backward is identically zero (tower_bwd_oracle's docstring) and the plant changed nothing
    agg_row0_residual_missing  (G) tensor spatial_attn_agg.cls_token 156
    wgrad_last_chunk_dropped   (G) attn.qkv.weight tensor 12.4, block 18.8 (33 of 1 569 rows left out)
  two segments, two blocks, the tower MLPs on the fused fc1 + GELU arm, the float32 draw (the two tests at the end; what the GPU file's two exemptions point to):
    gain 2: sums 0.61 - 0.78, means 0.64 - 0.90, the CLS rows 0.71 - 0.90, (G) 0.75 / 0.81; patch rows over the per-row bar, of 3 072: time 9 / 9, space 9 / 6, MLP 41 / 74
      (block 0 / 1; worst 1.61); none of the 64 side rows (worst 0.97).  At gain 1 no row of any branch (worst 0.78).
    gain 1, worst block ratio per 128-row block of the time qkv weight gradient:
      blocks.0  0.67 0.67 0.64 0.64 0.64 0.64 | 0.67 0.68 0.64 0.67 0.66 0.64 | 0.57 0.56 0.61 0.53 0.57 0.61
      blocks.1  0.82 0.74 0.69 0.60 0.62 0.67 | 0.85 0.75 0.70 0.65 0.61 0.70 | 0.62 0.60 0.62 0.69 0.63 0.63      (q rows | k rows | v rows)
      Row blocks 0 and 6 of the last block stand clear of the other sixteen, all below the bar: the same pattern as the trainer's, not an excess.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import attention_bwd_oracle as ABO  # noqa: E402
import tower_block_oracle as TB  # noqa: E402
import tower_bwd_oracle as O  # noqa: E402
from oracle import synchformer_cpu as SC  # noqa: E402

SEED = 1337
_CACHE = {}
# plant -> (configuration, where it must show: branch keys for (A), parameter-name fragments for (G))
EXPECT = {
    'dp_wrong_site': ('B', [(0, 'space'), (0, 'time')], ['blocks.0.attn.proj', 'blocks.0.attn.qkv']),
    'bias_unscaled': ('B', [], ['blocks.0.mlp.fc2.bias']),
    'stale_branch_head': ('A', [(0, 'space'), (0, 'time')], ['blocks.0.attn.proj', 'blocks.0.attn.qkv']),
    'cls_kv_group_missing': ('A', [(0, 'space')], ['blocks.0.attn.qkv']),
    'cls_kv_group_missing_time': ('A', [(0, 'time')], ['blocks.0.timeattn.qkv', 'vfeat_extractor.cls_token']),
    'cls_dq_first_group_only': ('A', [(0, 'time')], ['blocks.0.timeattn.qkv']),
    'agg_row0_residual_missing': ('A', [], ['spatial_attn_agg.cls_token']),
    'wgrad_last_chunk_dropped': ('A', [], ['blocks.0.attn.qkv.weight']),
}


def _sd():
    from synchformer_amd import synth
    return _CACHE.setdefault('sd', synth.make_state_dict(SEED, gain=1.0, vis_depth=1, aud_depth=1, sync_depth=1))


def _vis(cfg):
    """dict(sdp, x, dout, dps, exact, stepped, draw) of a visual configuration."""
    if ('vis', cfg) not in _CACHE:
        from synchformer_amd import synth
        n = 1 if cfg == 'A' else 2
        sdp = O.prepare_sd(_sd(), O.V)
        x = TB.frontend(synth.make_video_u8(1, n, SEED))
        dout = O.make_dout(n * 8, 11)
        k = 1.0 / 0.7
        dps = None if cfg == 'A' else [(torch.tensor([k, 0.0], dtype=torch.float64), torch.tensor([0.0, k], dtype=torch.float64))]
        c = dict(sdp=sdp, x=x, dout=dout, dps=dps, n=n)
        c['exact'] = O.exact_visual(sdp, x, 1, dout, dps)
        c['stepped'] = O.stepped_visual(sdp, x, 1, dout, dps)
        c['draw'] = O.stepped_visual(sdp, x, 1, dout, dps, dtype=torch.float32)
        _CACHE[('vis', cfg)] = c
    return _CACHE[('vis', cfg)]


def _aud():
    if 'aud' not in _CACHE:
        from synchformer_amd import synth
        sdp = O.prepare_sd(_sd(), O.A)
        spec = O.spec_frontend(synth.make_spectrogram(1, 2, SEED))
        dout = O.make_dout(2 * 6, 12)
        c = dict(sdp=sdp, spec=spec, dout=dout, n=2)
        c['exact'] = O.exact_audio(sdp, spec, 1, dout)
        c['stepped'] = O.stepped_audio(sdp, spec, 1, dout)
        c['draw'] = O.stepped_audio(sdp, spec, 1, dout, dtype=torch.float32)
        _CACHE['aud'] = c
    return _CACHE['aud']


def _site(c, branch):
    """The DropPath vector of a visual branch's own site (None: never dropped)."""
    if c.get('dps') is None or branch[1] == 'time':
        return None
    return c['dps'][branch[0]][0 if branch[1] == 'space' else 1]


def _judge(c, eng, tower='vis'):
    """(rows: branch -> check_rows, grads: check_grads) of `eng` against the configuration's exact and stepped models."""
    ex, st = c['exact'], c['stepped']
    rows = {}
    for b in ex.G:
        cl = O.vis_classes(c['n'], _site(c, b)) if tower == 'vis' else O.aud_classes(c['n'])
        rows[b] = O.check_rows(eng.G[b].to(torch.float64), ex.G[b], st.G[b], cl)
    return rows, O.check_grads(eng.grads, ex.grads, st.grads, st.F)


def _rel(a, b, scale=None):
    return ((a - b).norm() / max(b.norm().item(), scale or 0.0, 1e-300)).item()


def _peers(grads):
    pk = {}
    for t in grads.values():
        pk[t.numel()] = max(pk.get(t.numel(), 0.0), t.norm().item())
    return pk


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_split_forward_is_the_oracles_forward():
    """visual_forward_split / audio_forward_split restate divided_block / ast_layer at their residual additions: equal to motionformer_segments (with DropPath
    vectors) and ast_segments in float64 to 1e-12."""
    c, a = _vis('B'), _aud()
    with torch.no_grad():
        out, _ = O.visual_forward_split(c['sdp'], c['x'], 1, c['dps'])
        ref = SC.motionformer_segments(c['x'], c['sdp'], depth=1, drop_path=c['dps']).reshape(-1, O.D)
        oa, _ = O.audio_forward_split(a['sdp'], a['spec'], 1)
        ra = SC.ast_segments(a['spec'].transpose(1, 2), a['sdp'], depth=1).reshape(-1, O.D)
    print(f'split forward: visual {_rel(out, ref):.2e} audio {_rel(oa, ra):.2e}')
    assert _rel(out, ref) < 1e-12 and _rel(oa, ra) < 1e-12


@pytest.mark.parametrize('cfg', ['A', 'B', 'aud'])
def test_unrounded_stepped_equals_exact(cfg):
    """rnd=False: every rounding is the identity; out, every G_b and every parameter gradient equal float64 autograd to 1e-10 (relative to the tensor, or for a
    gradient that is mathematically zero - the key biases, whose shift leaves a softmax unchanged - to the largest gradient of the same size)."""
    if cfg == 'aud':
        c = _aud()
        st = O.stepped_audio(c['sdp'], c['spec'], 1, c['dout'], rnd=False)
    else:
        c = _vis(cfg)
        st = O.stepped_visual(c['sdp'], c['x'], 1, c['dout'], c['dps'], rnd=False)
    ex = c['exact']
    assert set(st.grads) == set(ex.grads) and set(st.G) == set(ex.G)
    pk = _peers(ex.grads)
    worst = max([_rel(st.out, ex.out)] + [_rel(st.G[b], ex.G[b]) for b in ex.G if ex.G[b].norm() > 0] + [_rel(st.grads[k], ex.grads[k], pk[ex.grads[k].numel()]) for k in ex.grads])
    print(f'{cfg}: stepped(rnd=False) vs exact, worst relative deviation {worst:.2e}')
    assert worst < 1e-10
    for b in ex.G:                                                            # a dropped branch adds exactly nothing
        if ex.G[b].norm() == 0:
            assert st.G[b].norm() == 0


@pytest.mark.parametrize('cfg', ['B', 'aud'])
def test_exact_agrees_with_fp32_autograd(cfg):
    """exact (float64, bf16-rounded GEMM weights) against float32 autograd through oracle.synchformer_cpu's own top-level function on the same weights: every
    parameter gradient to 1e-4 of its norm (or of the largest gradient of its size) - fp32's 6e-8 through sums of up to 3072 terms and two LayerNorm backwards."""
    c = _vis('B') if cfg == 'B' else _aud()
    leaves = {k: t.float().requires_grad_(True) for k, t in c['sdp'].items()}
    if cfg == 'B':
        dps = [tuple(t.float() for t in c['dps'][0])]
        out = SC.motionformer_segments(c['x'].float(), leaves, depth=1, drop_path=dps).reshape(-1, O.D)
    else:
        out = SC.ast_segments(c['spec'].float().transpose(1, 2), leaves, depth=1).reshape(-1, O.D)
    (out * c['dout'].float()).sum().backward()
    ex = c['exact'].grads
    pk = _peers(ex)
    rows = sorted(((_rel(leaves[k].grad.double(), ex[k], pk[ex[k].numel()]), k) for k in ex if leaves[k].grad is not None), reverse=True)
    print(f'{cfg}: exact vs fp32 autograd, worst {rows[0][0]:.2e} {rows[0][1]}, median {rows[len(rows) // 2][0]:.2e}')
    assert rows[0][0] < 1e-4, rows[0]


@pytest.mark.parametrize('cfg', ['A', 'B', 'aud'])
def test_another_draw_passes_with_room(cfg):
    """The stepped model in float32 - the same rounding points, other draws - passes (A) row / sum / mean and (G) tensor / block."""
    c = _aud() if cfg == 'aud' else _vis(cfg)
    rows, grads = _judge(c, c['draw'], 'aud' if cfg == 'aud' else 'vis')
    for b, r in rows.items():
        w, cl = O.worst_rows(r)
        lv = O.noise_levels(c['exact'].G[b], c['stepped'].G[b], O.aud_classes(c['n']) if cfg == 'aud' else O.vis_classes(c['n'], _site(c, b)))
        print(f'{cfg} {b}: (A) worst {w:.3f} in {cl}; ' + ' '.join(f'{k} row {v[0]:.2f} sum {v[1]:.2f} mean {v[2]:.2f} noise {lv[k]:.1e}' for k, v in r.items()))
        assert w <= 1.0, (b, r)
    (t, tk), (bl, bk) = O.worst_grads(grads)
    print(f'{cfg}: (G) worst tensor {t:.3f} {tk}; worst block {bl:.3f} {bk}')
    assert t <= 1.0 and bl <= 1.0, (t, tk, bl, bk)


@pytest.mark.parametrize('plant', O.PLANTS)
def test_plant_is_rejected(plant):
    """Every plant exceeds a bar, in a branch or tensor named for it (EXPECT)."""
    cfg, branches, frags = EXPECT[plant]
    c = _vis(cfg)
    eng = O.stepped_visual(c['sdp'], c['x'], 1, c['dout'], c['dps'], plant=plant)
    rows, grads = _judge(c, eng)
    hits = []
    for b in branches:
        for cl, v in rows[b].items():
            for nm, r in zip(('row', 'sum', 'mean'), v):
                if r > 1.0:
                    hits.append(f'(A) {nm} {b} {cl} {r:.3g}')
    for k, v in grads.items():
        if any(f in k for f in frags):
            if v[0] > 1.0:
                hits.append(f'(G) tensor {k} {v[0]:.3g}')
            if v[1] is not None and v[1] > 1.0:
                hits.append(f'(G) block {k} {v[1]:.3g}')
    print(f'{plant}: ' + ('; '.join(hits) if hits else 'NOT CAUGHT'))
    assert hits, plant


@pytest.mark.parametrize('geometry,clsq', [((3, 1, 5, 1, 5, 0), False), ((3, 1, 1, 3, 5, 0), True), ((2, 0, 4, 1, 4, -1), False), ((2, 0, 1, 2, 3, 7), True),
                                           ((1, 2, 1, 1, 1, 0), True)])
def test_attention_bwd_reference_matches_float64_autograd(geometry, clsq):
    """The moved grouped_attention_bwd_ref equals float64 autograd through the independently written forward to 1e-12 of the gradient's largest element, its emulation
    stays within its own element bars, and the group partials it now hands out sum to the reduced CLS rows."""
    G, row0, gs, ts, T, cls_row = geometry
    R = max(row0 + (G - 1) * gs + (T - 1) * ts, cls_row) + 2
    g = torch.Generator().manual_seed(3)
    q, k, v, dO = [(torch.randn(2, R, 3, 64, generator=g) * 0.8).to(ABO.BF).double().requires_grad_(True) for _ in range(4)]
    out = ABO._forward_autograd(q, k, v, geometry, 0.125, clsq)
    gq, gk, gv = torch.autograd.grad((out * dO.detach()).sum(), (q, k, v))
    ref = ABO.grouped_attention_bwd_ref(q.detach(), k.detach(), v.detach(), dO.detach(), geometry, 0.125, clsq=clsq)
    for name, a in (('dq', gq), ('dk', gk), ('dv', gv)):
        err = (ref['full'][name] - a).abs().max().item()
        assert err <= 1e-12 * max(a.abs().max().item(), 1.0), (name, err)
    for name in ('dq_tok', 'dk_tok', 'dv_tok', 'dk_cls', 'dv_cls', 'dq_cls'):
        if name in ref:
            sec = ref[name]
            assert ((sec.emu - sec.ref).abs() <= sec.bar).all(), name
            assert (sec.bar > 0).all(), name
    for x, part in ref['partials'].items():
        assert torch.equal(ABO._rb(ABO._rb(part).sum(1)), ref[x + '_cls'].emu), x


def _two_blocks(gain):
    """(exact, stepped, float32 draw) of two segments through two blocks, the tower MLPs on the fused fc1 + GELU arm as in the GPU cases (Arm.dual)."""
    from synchformer_amd import synth
    sdp = O.prepare_sd(synth.make_state_dict(SEED, gain=gain, vis_depth=2, aud_depth=1, sync_depth=1), O.V)
    x, dout = TB.frontend(synth.make_video_u8(1, 2, SEED)), O.make_dout(16, 101)
    arm = O.Arm(dual=True)
    return O.exact_visual(sdp, x, 2, dout), O.stepped_visual(sdp, x, 2, dout, arm=arm), O.stepped_visual(sdp, x, 2, dout, dtype=torch.float32, arm=arm)


def test_per_row_bar_at_gain_2_is_not_a_bound_on_another_draw():
    """The basis of the GPU file's v_gain2 exemption, measured without an engine: at gain 2 (two segments, two blocks) the stepped model in float32 passes the class
    sums, the segment means, (G) and the per-row bar of the CLS class, but patch rows of every branch - most in the MLP branches - exceed 1.5 max(noise(r), median):
    the per-row noise is a few-draw quantity there.  The side class (64 rows here, to the trainer ordinary patch rows) is printed; the draw does not exceed in it."""
    ex, st, dr = _two_blocks(2.0)
    over = {}
    for b in ex.G:
        cl = O.vis_classes(2)
        r = O.check_rows(dr.G[b].double(), ex.G[b], st.G[b], cl)
        err, noise = (dr.G[b].double() - ex.G[b]).norm(dim=-1), (st.G[b] - ex.G[b]).norm(dim=-1)
        over[b] = {k: int((err[m] > O.MARGIN_A * torch.maximum(noise[m], noise[m].median())).sum()) for k, m in cl.items()}
        print(f'gain 2 {b}: ' + ' '.join(f'{k} row {v[0]:.2f} sum {v[1]:.2f} mean {v[2]:.2f} rows over the bar {over[b][k]} of {int(cl[k].sum())};' for k, v in r.items()))
        assert all(v[1] <= 1.0 and v[2] <= 1.0 for v in r.values()), (b, r)
        assert r['cls'][0] <= 1.0, (b, r)
    (t, tk), (bl, bk) = O.worst_grads(O.check_grads(dr.grads, ex.grads, st.grads, st.F))
    print(f'gain 2: (G) worst tensor {t:.3f} {tk}; worst block {bl:.3f} {bk}')
    assert t <= 1.0 and bl <= 1.0
    assert all(over[b]['patch'] > 0 for b in ex.G), over


def test_last_time_qkv_gradient_has_few_draw_row_blocks():
    """The basis of the GPU file's v_n7 exemption, measured without an engine: at gain 1 (two segments, two blocks) the float32 draw's per-block ratios of
    blocks.1.timeattn.qkv.weight are highest in row blocks 0 and 6 (the q rows and the k rows of heads 0 and 1), clear of the other sixteen - the pattern the
    trainer shows - while block 0's tensor is flat.  The draw itself stays under the bar: it shows where the noise holds few draws, not an excess."""
    ex, st, dr = _two_blocks(1.0)
    rb = {}
    for i in (0, 1):
        k = f'{O.V}.blocks.{i}.timeattn.qkv.weight'
        rb[i] = (O._blocks(dr.grads[k].double() - ex.grads[k]) / (O.MARGIN_A * O._blocks(st.grads[k] - ex.grads[k]))).max(1).values.tolist()
        print(f'gain 1 {k}: worst block ratio per 128-row block ' + ' '.join(f'{v:.2f}' for v in rb[i]))
    rest = [v for j, v in enumerate(rb[1]) if j not in (0, 6)]
    assert min(rb[1][0], rb[1][6]) > max(rest), rb[1]
    assert max(rb[1]) <= 1.0 and max(rb[0]) <= 1.0
    assert min(rb[1][0], rb[1][6]) > max(rb[0]), (rb[0], rb[1])                # block 0's tensor has no such row blocks
