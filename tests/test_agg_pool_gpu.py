"""GPU: sf_agg_cls_pool (csrc/sf_agg_pool.hip) - the aggregator layer's CLS-query attention pooled in one pass over the residual stream - and the periodic residual
of sf_gemm_res_ln768_periodic (csrc/sf_gemm_ln.hip).

Pooled attention.  Every case builds a float64 reference on the host from the same fp32 X and the same (bf16-rounded) weights: plain final LayerNorm -> [cls_token;
rows] -> norm1 -> qkv -> softmax of row 0 over the kept keys -> P V, and runs the path the engine took before through the existing ops (layernorm, layernorm, gemm,
attention_cls).  The new path is sf_agg_cls_pool + the per-head value projection (12 strided ops.gemm calls with [W_v[h] | W_v[h]] on G[:, h], which the launch writes
as bf16 hi | lo), so both paths end in the same bf16 (n_seq, 768) attention output.  The bar is measured, not fixed: the new path's rel-RMS and max |delta| against float64 must be <= 1.25 x the old path's on the same
inputs (the pooled form has fewer rounding points; the 1.25 leaves room for its bf16 P operand).  Both figures are printed.  test_folded_projection checks the form
the engine uses after the pool (one GEMM against W_o blockdiag(W_v), every block against hi and lo, K = 18432) against the old out-projection in the same way.

The launch is one workgroup per sequence (not persistent), so a many-segment case would add nothing a one-segment case does not run.  Its key chunks are 16 wide with
the CLS key in slot 0: n_tok 15 / 16 / 31 / 32 / 33 put the last key on both sides of a chunk edge, 196 = 12 chunks + 5 keys.

Periodic residual.  M = 3 x 1569 rows (128-row tiles cross the sequence boundaries at offsets 33, 66 and 99), K in {768, 1536}, and a period beyond M: X and Y must be
bit-identical to sf_broadcast_rows768 followed by sf_gemm_res_ln768 in place.

Every case prints its four figures (pytest -s): rel-RMS and max |delta| of the new and of the old path against float64, and their ratios (bar 1.25)."""
import math

import pytest
import torch

BF = torch.bfloat16
D, H, HD = 768, 12, 64
EPS_A, EPS_B = 1e-6, 1e-6
VIS = dict(seq_rows=1569, row0=1, n_groups=8, group_stride=196, tok_stride=1, n_tok=196)
AUD = dict(seq_rows=74, row0=2, n_groups=6, group_stride=1, tok_stride=6, n_tok=12)
RATIO = 1.25


def _ops():
    from synchformer_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rb(x):
    return x.to(torch.float32).to(BF).to(torch.float64)


def _ln64(x, g, b, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * g + b


def _desc(n_tok, n_groups=2):
    return dict(seq_rows=1 + n_groups * n_tok, row0=1, n_groups=n_groups, group_stride=n_tok, tok_stride=1, n_tok=n_tok)


def _token_rows(desc, n_seg):
    """(n_seq, n_tok) int64: the X row of token t of sequence sq = segment * n_groups + g."""
    seg = torch.arange(n_seg).view(-1, 1, 1) * desc['seq_rows']
    g = torch.arange(desc['n_groups']).view(1, -1, 1) * desc['group_stride']
    t = torch.arange(desc['n_tok']).view(1, 1, -1) * desc['tok_stride']
    return (seg + desc['row0'] + g + t).reshape(n_seg * desc['n_groups'], desc['n_tok'])


def _weights(seed, w_scale=0.04):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    w = dict(cls=0.5 * r(D), g_a=1.0 + 0.1 * r(D), b_a=0.1 * r(D), g_b=1.0 + 0.1 * r(D), b_b=0.1 * r(D),
             w_in=(w_scale * r(3 * D, D)).to(BF).float(), b_in=0.1 * r(3 * D), w_o=(0.04 * r(D, D)).to(BF).float(), b_o=0.1 * r(D))
    return w


def _reference(X, w, desc, n_seg, keep):
    """float64: att (n_seq, 768) = row 0 of the aggregator's attention, the scores of the token keys (n_seq, H, n_tok) in natural-log units, and zn_cls."""
    rows = _token_rows(desc, n_seg)
    n_seq, n_tok = rows.shape
    f = lambda k: w[k].to(torch.float64)
    z = _ln64(X.to(torch.float64)[rows.reshape(-1)], f('g_a'), f('b_a'), EPS_A).float().to(torch.float64).view(n_seq, n_tok, D)      # (the Z buffer was fp32)
    z = torch.cat([f('cls').view(1, 1, D).expand(n_seq, 1, D), z], 1)
    zn = _rb(_ln64(z, f('g_b'), f('b_b'), EPS_B))
    w_in, b_in = f('w_in'), f('b_in')
    q = (zn[:, 0] @ w_in[:D].T + b_in[:D]).view(n_seq, H, HD)
    k = (zn @ w_in[D:2 * D].T + b_in[D:2 * D]).view(n_seq, n_tok + 1, H, HD)
    v = (zn @ w_in[2 * D:].T + b_in[2 * D:]).view(n_seq, n_tok + 1, H, HD)
    s = torch.einsum('nhd,njhd->nhj', q, k) * HD ** -0.5
    if keep is not None:
        kk = torch.cat([torch.ones(n_seq, 1, dtype=torch.bool), keep[rows.reshape(-1)].view(n_seq, n_tok) != 0], 1)
        s = s.masked_fill(~kk.view(n_seq, 1, n_tok + 1), -math.inf)
    p = torch.softmax(s, -1)
    att = torch.einsum('nhj,njhd->nhd', p, v).reshape(n_seq, D)
    return att, s[:, :, 1:], zn[0, 0]


def _old_path(X, w, desc, n_seg, keep, dev):
    """The launches the engine used: final norm into Z = [cls; rows], norm1, the qkv GEMM, attention_cls for row 0."""
    ops = _ops()
    rows = _token_rows(desc, n_seg)
    n_seq, n_tok = rows.shape
    L = n_tok + 1
    d = lambda k, dt=torch.float32: w[k].to(dev, dt).contiguous()
    xs = X[rows.reshape(-1)].to(dev).contiguous()                   # the gather the row maps did
    zt = torch.empty(n_seq * n_tok, D, device=dev, dtype=torch.float32)
    if n_tok:
        ops.layernorm(xs, d('g_a'), d('b_a'), zt, EPS_A)
    Z = torch.cat([d('cls').view(1, 1, D).expand(n_seq, 1, D), zt.view(n_seq, n_tok, D)], 1).reshape(n_seq * L, D).contiguous()
    zn = torch.empty(n_seq * L, D, device=dev, dtype=BF)
    ops.layernorm(Z, d('g_b'), d('b_b'), zn, EPS_B)
    qkv = torch.empty(n_seq * L, 3 * D, device=dev, dtype=BF)
    ops.gemm(zn, d('w_in', BF), d('b_in'), qkv)
    zkeep = None
    if keep is not None:
        zkeep = torch.ones(n_seq, L, dtype=torch.uint8)
        zkeep[:, 1:] = keep[rows.reshape(-1)].view(n_seq, n_tok)
        zkeep = zkeep.reshape(-1).to(dev)
    att = torch.empty(n_seq, D, device=dev, dtype=BF)
    ops.attention_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], att, n_seq=n_seq, q_seq_rows=L, q_row=0, kv_seq_rows=L, kv_row0=0, n_keys=L,
                      out_seq_rows=1, out_row=0, heads=H, head_dim=HD, scale=HD ** -0.5, key_keep=zkeep)
    return att


def _operands(w, dev):
    from synchformer_amd.engine import agg_cls_operands
    u, c, zn_cls, w_vo, b_vo = agg_cls_operands(w['cls'], w['g_b'], w['b_b'], w['w_in'], w['b_in'], w['w_o'], w['b_o'], heads=H, eps=EPS_B)
    return dict(u=u.to(dev), c=c.to(dev), zn_cls=zn_cls.to(dev)), w_vo.to(dev, BF), b_vo.to(dev)


def _pool(X_dev, w, desc, n_seg, keep_dev, dev, canary=True):
    ops = _ops()
    n_seq = n_seg * desc['n_groups']
    cq, _, _ = _operands(w, dev)
    d = lambda k: w[k].to(dev).contiguous()
    G = torch.full((n_seq, 2 * H * D), 3.0, device=dev, dtype=BF) if canary else torch.empty(n_seq, 2 * H * D, device=dev, dtype=BF)
    ops.agg_cls_pool(X_dev, G, n_seq=n_seq, norm_a=(d('g_a'), d('b_a')), eps_a=EPS_A, norm_b=(d('g_b'), d('b_b')), eps_b=EPS_B, key_keep=keep_dev, **cq, **desc)
    return G


def _value_proj(G, w, dev):
    """att[:, 64 h .. 64 h + 63] = (G_hi[:, h] + G_lo[:, h]) W_v[h]^T + b_v[h]: twelve strided GEMMs (K = 2 x 768, the weight twice) into the bf16 attention output
    the old path ends in."""
    ops = _ops()
    w_v, b_v = w['w_in'][2 * D:].to(dev, BF).contiguous(), w['b_in'][2 * D:].to(dev).contiguous()
    att = torch.empty(G.shape[0], D, device=dev, dtype=BF)
    for h in range(H):
        ops.gemm(G[:, 2 * h * D:2 * (h + 1) * D], w_v[h * HD:(h + 1) * HD].repeat(1, 2), b_v[h * HD:(h + 1) * HD], att[:, h * HD:(h + 1) * HD])
    return att


def _errs(got, ref):
    e = got.detach().cpu().to(torch.float64) - ref
    return float(e.norm() / ref.norm()), float(e.abs().max())


def _compare(what, X, w, desc, n_seg, keep=None):
    dev = torch.device('cuda:0')
    ref, s_ref, _ = _reference(X, w, desc, n_seg, keep)
    old = _old_path(X, w, desc, n_seg, keep, dev)
    G = _pool(X.to(dev), w, desc, n_seg, None if keep is None else keep.to(dev), dev)
    new = _value_proj(G, w, dev)
    torch.cuda.synchronize()
    assert torch.isfinite(G.float()).all()
    (r_new, m_new), (r_old, m_old) = _errs(new, ref), _errs(old, ref)
    print(f'\n[agg_pool] {what}: rel-RMS new {r_new:.3e} old {r_old:.3e} ({r_new / r_old:.2f}x)   max|d| new {m_new:.3e} old {m_old:.3e} ({m_new / m_old:.2f}x)')
    assert r_new <= RATIO * r_old, (what, r_new, r_old)
    assert m_new <= RATIO * m_old, (what, m_new, m_old)
    return G, s_ref


def _x(seed, rows, scale=1.0):
    return scale * torch.randn(rows, D, generator=_gen(seed))


@pytest.mark.gpu
def test_visual_descriptor_one_segment(gpu):
    _compare('visual, 1 segment', _x(1, 1569), _weights(2), VIS, 1)


@pytest.mark.gpu
def test_audio_descriptor(gpu):
    _compare('audio, 2 segments', _x(3, 2 * 74), _weights(4), AUD, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('n_tok', [1, 15, 16, 31, 32, 33, 196])
def test_sequence_lengths(gpu, n_tok):
    desc = _desc(n_tok)
    _compare(f'n_tok {n_tok}', _x(10 + n_tok, 2 * desc['seq_rows']), _weights(5), desc, 2)


@pytest.mark.gpu
def test_large_rows_with_outlier_channels(gpu):
    X = _x(20, 1569, 10.0)
    X[:, [5, 300, 767]] *= 30.0
    X[:, 100] += 200.0
    _compare('rows ~10, outlier channels', X, _weights(21), VIS, 1)


def _ramp_case(seed, descending):
    """Scores that rise (fall) strictly along every sequence for every head: rows f + a_j e + noise with e a +-1 pattern, f a fixed unit-variance Gaussian pattern
    made orthogonal to e and to the ones vector (distinct magnitudes: the bf16 roundings of zn do not add up coherently), a_j monotone in j, identity norms, and
    W_k[h] = gamma q_h e^T / (|q_h|^2 768): s_j = scale gamma (e . zn_j) / 768 with e . zn_j / 768 = a_j / sqrt(1 + a_j^2) up to noise and rounding."""
    g = _gen(seed)
    desc = _desc(196, n_groups=2)
    w = _weights(seed + 1)
    w['g_a'], w['b_a'], w['g_b'], w['b_b'] = torch.ones(D), torch.zeros(D), torch.ones(D), torch.zeros(D)
    i = torch.arange(D)
    e = torch.where(i % 2 == 0, 1.0, -1.0)
    f = torch.randn(D, generator=g, dtype=torch.float64)
    f = f - (f @ e.to(torch.float64) / D) * e.to(torch.float64)
    f = f - f.mean()
    f = (f / f.std(unbiased=False)).float()
    a = torch.linspace(0.02, 1.0, 196)
    if descending:
        a = a.flip(0)
    rows = _token_rows(desc, 1)
    X = 1e-4 * torch.randn(desc['seq_rows'], D, generator=g)
    X[rows.reshape(-1)] += f + a.repeat(2).view(-1, 1) * e
    cls64 = w['cls'].to(torch.float64)
    zn_cls = _rb(_ln64(cls64, torch.ones(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64), EPS_B))
    q = (zn_cls @ w['w_in'][:D].to(torch.float64).T + w['b_in'][:D].to(torch.float64)).view(H, HD)
    gamma = 40.0 / HD ** -0.5
    w_k = gamma * q.view(H, HD, 1) * e.to(torch.float64).view(1, 1, D) / ((q * q).sum(1).view(H, 1, 1) * D)
    w['w_in'][D:2 * D] = w_k.reshape(D, D).to(BF).float()
    w['b_in'][D:2 * D] = 0.0
    return X, w, desc


@pytest.mark.gpu
@pytest.mark.parametrize('descending', [False, True])
def test_monotone_scores(gpu, descending):
    """Ascending scores move the running maximum (and rescale the accumulators) in every chunk; descending scores never do after the first."""
    X, w, desc = _ramp_case(30, descending)
    _, s = _compare('descending scores' if descending else 'ascending scores', X, w, desc, 1)
    d = s[:, :, 1:] - s[:, :, :-1]
    assert bool((d < 0).all() if descending else (d > 0).all())
    assert float(s.max() - s.min()) > 20.0                           # a range that matters: the first and last keys differ by e^20 in weight


@pytest.mark.gpu
def test_random_key_mask(gpu):
    keep = (torch.rand(1569, generator=_gen(40)) >= 0.2).to(torch.uint8)
    _compare('20 % of the keys dropped', _x(41, 1569), _weights(42), VIS, 1, keep)


@pytest.mark.gpu
def test_sequence_with_every_patch_key_dropped(gpu):
    """Sequence 3 keeps only the CLS key: its pooled rows are zn_cls (bf16) for every head, bit for bit (hi = zn_cls, lo = 0) - the projection of zn_cls after the
    value GEMM."""
    dev = torch.device('cuda:0')
    keep = (torch.rand(1569, generator=_gen(50)) >= 0.2).to(torch.uint8)
    keep[1 + 3 * 196:1 + 4 * 196] = 0
    X, w = _x(51, 1569), _weights(52)
    G, _ = _compare('one sequence fully masked', X, w, VIS, 1, keep)
    cq, _, _ = _operands(w, dev)
    want = torch.stack([cq['zn_cls'].to(BF), torch.zeros(D, device=dev, dtype=BF)]).view(1, 2, D).expand(H, 2, D)
    assert torch.equal(G[3].view(H, 2, D).view(torch.int16), want.contiguous().view(torch.int16))


@pytest.mark.gpu
def test_bit_identities(gpu):
    """An all-ones mask == no mask; two runs agree; a sequence run alone (n_seq = 1, its own descriptor) == the same sequence inside the batch."""
    dev = torch.device('cuda:0')
    X, w = _x(60, 2 * 1569).to(dev), _weights(61)
    a = _pool(X, w, VIS, 2, None, dev)
    b = _pool(X, w, VIS, 2, None, dev)
    c = _pool(X, w, VIS, 2, torch.ones(2 * 1569, device=dev, dtype=torch.uint8), dev)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    for sq in (0, 5, 11):
        seg, g = divmod(sq, 8)
        alone = dict(seq_rows=1569, row0=1 + g * 196, n_groups=1, group_stride=0, tok_stride=1, n_tok=196)
        one = _pool(X[seg * 1569:(seg + 1) * 1569], w, alone, 1, None, dev)
        assert torch.equal(one[0].view(torch.int16), a[sq].view(torch.int16)), sq
    keep = (torch.rand(2 * 1569, generator=_gen(62)) >= 0.2).to(torch.uint8).to(dev)
    m = _pool(X, w, VIS, 2, keep, dev)
    alone = dict(seq_rows=1569, row0=1 + 2 * 196, n_groups=1, group_stride=0, tok_stride=1, n_tok=196)
    one = _pool(X[1569:], w, alone, 1, keep[1569:].contiguous(), dev)
    assert torch.equal(one[0].view(torch.int16), m[10].view(torch.int16))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_folded_projection(gpu):
    """The engine's form after the pool - ONE GEMM of G (n_seq, 18432: hi | lo per head) against W_o blockdiag(W_v) with the biases and the cls_token residual folded into its bias -
    against the old path's out-projection with the residual, both against float64."""
    ops = _ops()
    dev = torch.device('cuda:0')
    X, w = _x(70, 1569), _weights(71)
    ref_att, _, _ = _reference(X, w, VIS, 1, None)
    f = lambda k: w[k].to(torch.float64)
    ref = ref_att @ f('w_o').T + f('b_o') + f('cls')
    att_old = _old_path(X, w, VIS, 1, None, dev)
    y_old = torch.empty(8, D, device=dev, dtype=torch.float32)
    res = w['cls'].to(dev).view(1, D).expand(8, D).contiguous()
    ops.gemm(att_old, w['w_o'].to(dev, BF), w['b_o'].to(dev), y_old, residual=res)
    G = _pool(X.to(dev), w, VIS, 1, None, dev)
    _, w_vo, b_vo = _operands(w, dev)
    y_new = torch.empty(8, D, device=dev, dtype=torch.float32)
    ops.gemm(G, w_vo.contiguous(), b_vo, y_new)
    torch.cuda.synchronize()
    (r_new, m_new), (r_old, m_old) = _errs(y_new, ref), _errs(y_old, ref)
    print(f'\n[agg_pool] folded projection: rel-RMS new {r_new:.3e} old {r_old:.3e} ({r_new / r_old:.2f}x)   max|d| new {m_new:.3e} old {m_old:.3e} ({m_new / m_old:.2f}x)')
    assert r_new <= RATIO * r_old and m_new <= RATIO * m_old


@pytest.mark.gpu
def test_rejected_arguments(gpu):
    ops = _ops()
    dev = torch.device('cuda:0')
    w = _weights(80)
    X = torch.zeros(74, D, device=dev)
    bad = dict(AUD, n_tok=13)                                        # the last token row would lie outside the sequence
    with pytest.raises((RuntimeError, AssertionError)):
        _pool(X, w, bad, 1, None, dev)
    with pytest.raises((RuntimeError, AssertionError)):
        ops.gemm_res_ln(torch.zeros(128, 768, device=dev, dtype=BF), torch.zeros(768, 768, device=dev, dtype=BF), None, torch.zeros(128, D, device=dev),
                        torch.ones(D, device=dev), torch.zeros(D, device=dev), torch.zeros(128, D, device=dev, dtype=BF), 1e-6,
                        residual=torch.zeros(32, D, device=dev), period=32)      # a tile could wrap twice


@pytest.mark.gpu
@pytest.mark.parametrize('K,period,kmajor', [(768, 1569, True), (1536, 1569, True), (1536, 1569, False), (768, 5000, True)])
def test_periodic_residual_bit_identical(gpu, K, period, kmajor):
    ops = _ops()
    dev = torch.device('cuda:0')
    g = _gen(90 + K + period)
    M = 3 * 1569
    a = torch.randn(M, K, generator=g).to(dev, BF)
    wt = (0.03 * torch.randn(D, K, generator=g)).to(dev, BF)
    wk = ops.kmajor_weight(wt) if kmajor else wt
    bias, gamma, beta = (0.1 * torch.randn(D, generator=g)).to(dev), (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
    table = torch.randn(period, D, generator=g).to(dev)
    x0 = torch.empty(M, D, device=dev)
    if period <= M:
        ops.broadcast_rows(x0, table, n_seq=M // period, dst_seq_rows=period)
    else:
        x0.copy_(table[:M])
    y0 = torch.zeros(M, D, device=dev, dtype=BF)
    ops.gemm_res_ln(a, wk, bias, x0, gamma, beta, y0, 1e-6)
    x1, y1 = torch.full((M, D), 7.0, device=dev), torch.zeros(M, D, device=dev, dtype=BF)
    ops.gemm_res_ln(a, wk, bias, x1, gamma, beta, y1, 1e-6, residual=table, period=period)
    torch.cuda.synchronize()
    assert torch.equal(x0.view(torch.int32), x1.view(torch.int32))
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))
