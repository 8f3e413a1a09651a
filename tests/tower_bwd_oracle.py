"""Float64 oracle of one Stage-1 tower's forward + backward as AVCLIPTrainer schedules them (tests/test_tower_bwd_gpu.py, tests/test_tower_bwd_oracle_cpu.py).
Pure torch, no kernel of the library: every function runs on the device its tensors live on.

The tower is driven from its aggregator output: dout (n 8, 768) visual / (n 6, 768) audio, fp32 values at unit RMS from a fixed generator (make_dout), is the
upstream gradient of _bwd_visual / _bwd_audio; the contrastive head and its conditioning stay out of the measurement.  Weights: prepare_sd - every GEMM weight
bf16-rounded (the trainer multiplies by self.b in the forward and, through _wT, in the dgrad), everything else the fp32 value, all widened to float64.

Two models:

  exact    float64 autograd through oracle.synchformer_cpu's own functions (patch_embed_3d, vis_pos_table, divided_attention, _ln / _lin / _gelu, agg_encoder_layer_cls;
           ast_patch_embed, _softmax_attn for the AST), the blocks split at their residual additions so that the stream X_j in front of every branch is a tensor
           with a gradient; the screen holds the split forward to divided_block / motionformer_segments / ast_segments themselves.  Nothing is rounded.  Returns every
           parameter gradient and, per residual branch b, G_b = dX_after_branch_backward - dX_before = X_j.grad - X_{j+1}.grad.
  stepped  the same computation as an explicit backward, branch by branch, every value rounded to bf16 where the trainer stores it:
             forward   patches (sf_im2col_video / sf_im2col_spec write bf16); every LayerNorm output that feeds a GEMM (ht, hs, h2, h1, the aggregator's zn, yn);
                       q | k | v; the attention outputs; the softmax weights where the launch packs its exponentials before P V (attn_mfma_kernel: n_tok > 8 - the
                       space groups with their CLS partials, the AST's 74 keys; not the 8-token time groups (attn_tiny64_kernel) nor the CLS rows of
                       sf_attention_cls / sf_attention_cls_stats / the aggregator (attn_cls64_kernel), fp32 up to the store); `pre` and `act`.
                       `act` = bf16(gelu(fp32 accumulator + bias)) where sf_gemm_bf16_gelu_dual runs (rows >= 8192; its epilogue packs acc + bias for `pre` and
                       applies gelu_erf4 to the same fp32 values, sf_gemm_pp.hip), = bf16(gelu(bf16 pre)) where sf_gelu_fwd reads the stored `pre` (Arm.dual).
                       Not rounded: the fp32 residual stream, the final norm's rows (written to the fp32 aggregator input Z).
             backward  dy_b = bf16(dp[segment] * dx) (sf_branch_grad, sf_layernorm768_bwd_branch, sf_cast_bf16 in the aggregator); dact, dpre (GELU derivative at
                       the saved bf16 `pre`), dh, dO_b (every dx_dtype=torch.bfloat16 dgrad); dqkv with the attention backward's inner packings and per-group bf16
                       partials of the CLS key's dk | dv and the CLS query's dq, summed by sf_reduce_groups_bf16 (attention_bwd_oracle.grouped_attention_bwd_ref:
                       round_mid for the 196- and 74-token group kernel, not for the tiny kernel; fwd_packs_p for the space CLS row); dtok.
                       SF_CLS_IN_GROUP=0 / fused_attn_bwd=False: the CLS query's backward is sf_attention_cls_bwd's accumulate pass - dq of the CLS row one bf16
                       rounding, dk | dv of every row a second rounding on top of the stored bf16 value.  fused_attn_bwd=False runs the group part through
                       attn_bwd_seq (P, dS bf16 before the second products): modelled with the group kernel's packings (round_mid) for both kinds and the AST -
                       the same number of bf16 roundings at the same places up to the order of delta's subtraction.
                       Weight gradients: products of the bf16 dY and the saved bf16 input.  Bias gradients: fp32 column sums of the scaled fp32 gradient where
                       sf_branch_grad / sf_layernorm768_bwd_branch / colsum(dy_f32) produce them (proj, fc2, output.dense, linear2, out_proj), sums of the bf16 dY
                       where the GEMM or sf_rowsum_bf16 does (qkv, fc1, query / key / value, in_proj, linear1, the patch embeddings).
                       Not rounded: the fp32 residual gradient dx, the fp32 dgrads (the aggregator's dzn, the AST's summed query / key / value dgrad), LayerNorm
                       parameter gradients (fp32 sums over the bf16 dh), the table sums.
           With rnd=False every rounding is the identity and stepped equals exact to 1e-10 relative on every returned tensor (the screen checks it).
           dtype=torch.float32 runs the whole model in float32 (the attention backward oracle stays float64 inside): another draw of the same roundings, the
           screen's stand-in for an engine.

Criteria (stated by the issue before any measurement; MARGIN_A = 1.5 is the forward oracle's constant):
  (A) per row of every G_b, rows split into the forward oracle's classes (CLS, side, patch; audio: cls = CLS + distillation, patch), kept and dropped segments of the
      branch's own DropPath site separately:  ||G_engine(r) - G_exact(r)|| <= 1.5 max(noise(r), median noise of the class), noise = ||G_stepped - G_exact||; the same bar
      on the class sums and on the per-segment class means.  F(r) = 0: every G_b row is a LayerNorm backward of a bf16 dh, its stepped noise vanishes only where the
      branch was dropped - there exact, stepped and engine are all exactly zero and the row passes iff the engine's is zero too.
  (G) per parameter tensor  ||g_engine - g_exact|| <= 1.5 ||g_stepped - g_exact|| + ||F||, and per 128 x 128 block of every weight matrix.
      F = 2^-24 x depth x sum of absolute terms, the fp32 term of the sums whose stepped noise can vanish:
        fp32 column sums of a branch head (proj / fc2 / output.dense / linear2 / out_proj biases): depth = train_tail_oracle.colsum_depth(rows, vec) - branch_grad_kernel
          (sf_train.hip: rows_per_blk / 32 rows per lane, 3 shuffle levels, 2 levels over the waves) + colsum_partials_kernel, the vector form of sf_colsum;
        table sums (cls_token, pos_embed, temp_embed, position_embeddings, distillation_token, the aggregators' cls_token): depth = the number of terms (sf_seqsum
          and the torch copies are taken as one chain: n segments, then 8 frames or 196 positions).
      Weight matrices, LayerNorm parameters and the bf16-summed biases have F = 0: they are sums over bf16-rounded factors whose noise does not vanish.
  No bar uses the trainer's output.  The forward oracle's criterion (B), against an fp32 "flip" variant, is not repeated: the forward screen found it no sharper than (A).

PLANTS: errors a wrong schedule branch would make, applied inside the stepped model, in the last block: its space branch (dp_wrong_site, stale_branch_head,
cls_kv_group_missing, wgrad_last_chunk_dropped on attn.qkv), its MLP head (bias_unscaled), its time branch (cls_dq_first_group_only: the CLS rows of dx are zero until
the last block's space backward has run - the final norm drops them - so the CLS query's backward of the last space branch is identically zero and a plant there
would change nothing; cls_kv_group_missing_time: one partial of 196 left out instead of one of 8), the aggregator (agg_row0_residual_missing).
"""
import math
import os
import sys
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(_HERE))
import attention_bwd_oracle as ABO  # noqa: E402
import tower_block_oracle as TB  # noqa: E402
import train_tail_oracle as TT  # noqa: E402
from oracle import synchformer_cpu as SC  # noqa: E402

D, FF, HEADS, HD = 768, 3072, 12, 64
VL, VP, FRAMES, NTOK, AGG_V = 1569, 1568, 8, 196, 197
AL, AP, ANF, ANT, AGG_A = 74, 72, 12, 6, 13
V, A = 'vfeat_extractor', 'afeat_extractor'
VAGG, AAGG = V + '.spatial_attn_agg', A + '.freq_attn_agg'
EPS_V, EPS_A = SC.EPS_VIS, SC.EPS_AST
F64 = torch.float64
U32 = 2.0 ** -24
MARGIN_A = TB.MARGIN_A
PLANTS = ('dp_wrong_site', 'bias_unscaled', 'stale_branch_head', 'cls_kv_group_missing', 'cls_kv_group_missing_time', 'cls_dq_first_group_only',
          'agg_row0_residual_missing', 'wgrad_last_chunk_dropped')
# the arm of the schedule that changes a rounding point: CLS query inside the group kernels, fused attention backward, fc1 + GELU in one launch (None: rows >= 8192)
Arm = namedtuple('Arm', 'cls_in_group fused_attn dual', defaults=(True, True, None))
Result = namedtuple('Result', 'out G grads F')


def prepare_sd(sd, tower, device='cpu'):
    """float64 state dict of one tower (V or A): GEMM weights bf16-rounded, the rest as it is; the unused 2-D patch embedding of the visual tower left out."""
    out = {}
    for k, t in sd.items():
        if not k.startswith(tower + '.') or k.startswith(V + '.patch_embed.'):
            continue
        gemm = (k.endswith('.weight') and t.dim() >= 2) or k.endswith('in_proj_weight')
        out[k] = (t.detach().to(torch.bfloat16) if gemm else t.detach()).to(F64).to(device)
    return out


def make_dout(rows, seed, device='cpu'):
    """(rows, 768) fp32 values at unit RMS from a fixed generator, as float64."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, D, generator=g, dtype=torch.float32).to(F64).to(device)


def spec_frontend(spec):
    """(B, S, 1, 128, 66) fp32 -> (B S, 128, 66) float64."""
    return spec.reshape(-1, spec.shape[-2], spec.shape[-1]).to(F64)


def last_chunk_start(M, N, K, n_cu=256):
    """First row of the last non-empty split-K chunk of FlatTrainer._lin_bwd's weight gradient: its chunking arithmetic (which lives inside _lin_bwd and cannot be
    called on its own) with the product's own _wgrad_split; n_cu = the MI355X's 256 compute units, _lin_bwd's default without a device."""
    from synchformer_amd.train import _wgrad_split
    m_pad = ((M + 63) // 64) * 64
    if M >= 8192 and N % 256 == 0 and K % 256 == 0:
        sp = max(1, n_cu // ((N // 256) * (K // 256)))
        kc = ((M + sp - 1) // sp + 127) // 128 * 128
    else:
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        split = _wgrad_split(tiles) if M >= 8192 else max(1, min(_wgrad_split(tiles), m_pad // 128))
        kc = ((m_pad // split + 63) // 64) * 64
    return ((M - 1) // kc) * kc


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _leaves(sdp):
    return {k: t.clone().requires_grad_(True) for k, t in sdp.items()}


def _finish(out, Xs, dout, leaves, names):
    for t in Xs:
        t.retain_grad()
    (out * dout).sum().backward()
    G = {nm: (Xs[j].grad - Xs[j + 1].grad).detach() for j, nm in enumerate(names)}
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).detach() for k, t in leaves.items()}
    return Result(out.detach(), G, grads, None)


def visual_forward_split(sd, x, depth, dps=None):
    """The visual tower through oracle.synchformer_cpu's functions, split at the residual additions: (aggregator rows (N 8, 768), [X_0, X after time 0, after space 0,
    after MLP 0, ..]).  dps: per block a (space, mlp) pair of per-segment scale vectors or None."""
    N = x.shape[0]
    tok = SC.patch_embed_3d(x, sd[V + '.patch_embed_3d.proj.weight'], sd[V + '.patch_embed_3d.proj.bias'])
    X = torch.cat([sd[V + '.cls_token'].expand(N, 1, -1), tok], 1) + SC.vis_pos_table(sd, V)
    Xs = [X]
    for i in range(depth):
        p = f'{V}.blocks.{i}'
        s_, m_ = dps[i] if dps is not None else (None, None)
        X = X + SC.divided_attention(SC._ln(X, sd, p + '.norm3', EPS_V), sd, p + '.timeattn', 'time')
        Xs.append(X)
        br = SC.divided_attention(SC._ln(X, sd, p + '.norm1', EPS_V), sd, p + '.attn', 'space')
        X = X + (br if s_ is None else br * s_.view(-1, 1, 1))
        Xs.append(X)
        br = SC._lin(SC._gelu(SC._lin(SC._ln(X, sd, p + '.norm2', EPS_V), sd, p + '.mlp.fc1')), sd, p + '.mlp.fc2')
        X = X + (br if m_ is None else br * m_.view(-1, 1, 1))
        Xs.append(X)
    xf = SC._ln(X[:, 1:], sd, V + '.norm', EPS_V)
    out = SC.agg_encoder_layer_cls(xf.reshape(N * FRAMES, NTOK, -1), sd, VAGG).reshape(N * FRAMES, D)
    return out, Xs


def audio_forward_split(sd, spec, depth):
    """The AST through oracle.synchformer_cpu's functions (ast_segments' own lines), split at the residual additions: (aggregator rows (N 6, 768), [X_0, after
    attention 0, after MLP 0, ..]).  spec (N, 128, 66)."""
    N = spec.shape[0]
    e = A + '.ast.embeddings'
    tok = SC.ast_patch_embed(spec.transpose(1, 2), sd[e + '.patch_embeddings.projection.weight'], sd[e + '.patch_embeddings.projection.bias'])
    X = torch.cat([sd[e + '.cls_token'].expand(N, 1, -1), sd[e + '.distillation_token'].expand(N, 1, -1), tok], 1)
    X = X + sd[e + '.position_embeddings'][:, :X.shape[1]]
    Xs = [X]
    for i in range(depth):
        p = f'{A}.ast.encoder.layer.{i}'
        y = SC._ln(X, sd, p + '.layernorm_before', EPS_A)
        hd = lambda nm: SC._lin(y, sd, f'{p}.attention.attention.{nm}').reshape(N, AL, HEADS, HD).transpose(1, 2)   # noqa: E731
        a = SC._softmax_attn(hd('query'), hd('key'), hd('value'), 1.0 / math.sqrt(HD))
        X = X + SC._lin(a.transpose(1, 2).reshape(N, AL, D), sd, p + '.attention.output.dense')
        Xs.append(X)
        X = X + SC._lin(SC._gelu(SC._lin(SC._ln(X, sd, p + '.layernorm_after', EPS_A), sd, p + '.intermediate.dense')), sd, p + '.output.dense')
        Xs.append(X)
    xf = SC._ln(X, sd, A + '.ast.layernorm', EPS_A)[:, 2:]
    per_t = xf.reshape(N, ANF, ANT, -1).transpose(1, 2).reshape(N * ANT, ANF, -1)
    out = SC.agg_encoder_layer_cls(per_t, sd, AAGG).reshape(N * ANT, D)
    return out, Xs


def vis_branches(depth):
    return [(i, b) for i in range(depth) for b in ('time', 'space', 'mlp')]


def aud_branches(depth):
    return [(i, b) for i in range(depth) for b in ('attn', 'mlp')]


def exact_visual(sdp, x, depth, dout, dps=None):
    leaves = _leaves(sdp)
    out, Xs = visual_forward_split(leaves, x, depth, dps)
    return _finish(out, Xs, dout, leaves, vis_branches(depth))


def exact_audio(sdp, spec, depth, dout):
    leaves = _leaves(sdp)
    out, Xs = audio_forward_split(leaves, spec, depth)
    return _finish(out, Xs, dout, leaves, aud_branches(depth))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stepped
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, sdp, rnd, plant, dtype, arm):
        assert plant is None or plant in PLANTS
        self.sd = {k: t.to(dtype) for k, t in sdp.items()}
        self.rnd, self.plant, self.dt, self.arm = rnd, plant, dtype, arm
        self.g, self.F = {}, {}
        self.st = TB._Step(self.sd, TB.Schedule('bf16'), rnd, None, None)

    def r16(self, x):
        return TB.rb(x) if self.rnd else x

    def w(self, name, wkey=None):
        w = self.sd[wkey or name + '.weight']
        return w.reshape(w.shape[0], -1)

    def lin(self, a, name, wkey=None, bkey=None):
        return a @ self.w(name, wkey).t() + self.sd[bkey or name + '.bias']

    def ln(self, x, name, eps):
        return torch.nn.functional.layer_norm(x, (D,), self.sd[name + '.weight'], self.sd[name + '.bias'], eps)

    def put(self, key, val, F=None):
        self.g[key] = val.reshape(self.sd[key].shape)
        if F is not None:
            self.F[key] = F.reshape(self.sd[key].shape)

    def ln_bwd(self, x, name, dy, eps):
        """dx of y = LayerNorm(x) given dy; fills the norm's parameter gradients."""
        mu = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
        xh = (x - mu) * rstd
        self.put(name + '.weight', (dy * xh).reshape(-1, D).sum(0))
        self.put(name + '.bias', dy.reshape(-1, D).sum(0))
        dxh = dy * self.sd[name + '.weight']
        return rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))

    def lin_bwd(self, name, dy_b, x_b, *, bias=True, need_dx=True, round_dx=True, wkey=None, bkey=None, drop_chunk=False):
        """Weight gradient dy^T x and (bias) the sum of the bf16 dY; returns the dgrad dy W, bf16-rounded where the trainer's GEMM writes bf16."""
        wkey = wkey or name + '.weight'
        w = self.w(name, wkey)
        dy2, x2 = dy_b.reshape(-1, w.shape[0]), x_b.reshape(-1, w.shape[1])
        if drop_chunk:
            r = last_chunk_start(dy2.shape[0], *w.shape)
            self.put(wkey, dy2[:r].t() @ x2[:r])
        else:
            self.put(wkey, dy2.t() @ x2)
        if bias:
            self.put(bkey or name + '.bias', dy2.sum(0))
        if not need_dx:
            return None
        dx = dy_b @ w
        return self.r16(dx) if round_dx else dx

    def head(self, dx, dp, bias_key, unscaled_bias=False):
        """Head of a residual branch's backward: dy_b = bf16(dp * dx), the output Linear's bias gradient = fp32 column sums of the scaled gradient."""
        sc = dx if dp is None else dx * dp
        src = dx if unscaled_bias else sc
        rows = dx.numel() // D
        self.put(bias_key, src.reshape(-1, D).sum(0), U32 * TT.colsum_depth(rows, True) * src.abs().reshape(-1, D).sum(0))
        return self.r16(sc)

    def mlp_fwd(self, x_in, ln, eps, fc1, fc2, dp=None, tower=True):
        rows = x_in.numel() // D
        # Arm.dual forces the arm of the TOWER MLPs only: an aggregator's MLP has n 8 / n 6 rows and never reaches sf_gemm_bf16_gelu_dual
        dual = tower and (self.arm.dual if self.arm.dual is not None else rows >= 8192)
        h2 = self.r16(self.ln(x_in, ln, eps))
        pre_f = self.lin(h2, fc1)
        pre = self.r16(pre_f)
        act = self.r16(_gelu(pre_f if dual else pre))
        br = self.lin(act, fc2)
        return x_in + (br if dp is None else br * dp), dict(x_in=x_in, h2=h2, pre=pre, act=act)

    def mlp_bwd(self, s, dy_b, ln, eps, fc1, fc2):
        dact = self.lin_bwd(fc2, dy_b, s['act'], bias=False)
        dpre = self.r16(dact * _dgelu(s['pre']))
        dh = self.lin_bwd(fc1, dpre, s['h2'])
        return self.ln_bwd(s['x_in'], ln, dh, eps)

    # ---- aggregator layer ---------------------------------------------------------------------------------------------------------------
    def agg_fwd(self, Z, p):
        n_seq, L = Z.shape[:2]
        zn = self.r16(self.ln(Z, p + '.norm1', EPS_V))
        qkv = self.r16(self.lin(zn, p, p + '.self_attn.in_proj_weight', p + '.self_attn.in_proj_bias'))
        hs = lambda t: t.reshape(n_seq, -1, HEADS, HD).transpose(1, 2)                  # noqa: E731  (n_seq, H, rows, 64)
        q, k, v = hs(qkv[:, :1, :D]), hs(qkv[..., D:2 * D]), hs(qkv[..., 2 * D:])
        att = self.r16((torch.softmax(0.125 * q @ k.mT, -1) @ v).transpose(1, 2).reshape(n_seq, D))
        y = Z[:, 0] + self.lin(att, p + '.self_attn.out_proj')
        out, m = self.mlp_fwd(y, p + '.norm2', EPS_V, p + '.linear1', p + '.linear2', tower=False)
        return out, dict(Z=Z, zn=zn, qkv=qkv, att=att, mlp=m)

    def agg_bwd(self, dout, s, p):
        Z = s['Z']
        n_seq, L = Z.shape[:2]
        dy = dout.to(self.dt)
        dy = dy + self.mlp_bwd(s['mlp'], self.head(dy, None, p + '.linear2.bias'), p + '.norm2', EPS_V, p + '.linear1', p + '.linear2')
        dy_b = self.head(dy, None, p + '.self_attn.out_proj.bias')
        dO_b = self.lin_bwd(p + '.self_attn.out_proj', dy_b, s['att'], bias=False)
        hs = lambda t: t.reshape(n_seq, -1, HEADS, HD).transpose(1, 2).reshape(n_seq * HEADS, -1, HD).to(F64)   # noqa: E731
        qkv = s['qkv']
        c = ABO._core(hs(qkv[:, :1, :D]), hs(qkv[..., D:2 * D]), hs(qkv[..., 2 * D:]), hs(dO_b.reshape(n_seq, 1, D)), 0.125, False)
        back = lambda t: t.reshape(n_seq, HEADS, -1, HD).transpose(1, 2).reshape(n_seq, -1, D).to(self.dt)      # noqa: E731
        dqkv = torch.zeros_like(qkv)
        dqkv[:, :1, :D], dqkv[..., D:2 * D], dqkv[..., 2 * D:] = back(c['dq']), back(c['dk']), back(c['dv'])
        dqkv = self.r16(dqkv)
        dzn = self.lin_bwd(p, dqkv, s['zn'], round_dx=False, wkey=p + '.self_attn.in_proj_weight', bkey=p + '.self_attn.in_proj_bias')
        dZ = self.ln_bwd(Z, p + '.norm1', dzn, EPS_V)
        if self.plant != 'agg_row0_residual_missing':
            dZ[:, 0] += dy
        self.put(p + '.cls_token', dZ[:, 0].sum(0), U32 * n_seq * dZ[:, 0].abs().sum(0))
        return dZ

    # ---- attention backward -------------------------------------------------------------------------------------------------------------
    def grouped_bwd(self, qkv, dO, geo, *, clsq, round_mid, fwd_packs_p, cls_pass, plant=None):
        """qkv (N, L, 2304), dO (N, L, 768) -> dqkv (N, L, 2304).  cls_pass: the CLS query's backward as sf_attention_cls_bwd's accumulate pass."""
        N, L = qkv.shape[:2]
        h4 = lambda t: t.reshape(N, L, HEADS, HD).to(F64)                               # noqa: E731
        q, k, v, d4 = h4(qkv[..., :D]), h4(qkv[..., D:2 * D]), h4(qkv[..., 2 * D:]), h4(dO)
        out = ABO.grouped_attention_bwd_ref(q, k, v, d4, geo, 0.125, clsq=clsq, round_mid=round_mid, fwd_packs_p=fwd_packs_p)
        cls_row = geo[5]
        if not self.rnd:
            full = out['full']
        else:
            full = {x: torch.zeros_like(q) for x in ('dq', 'dk', 'dv')}
            for x in full:
                full[x][:, out['idx']] = out[x + '_tok'].emu.permute(0, 1, 3, 2, 4)
            if cls_row >= 0:
                for x in ('dk', 'dv'):
                    full[x][:, cls_row] = out[x + '_cls'].emu
            if clsq:
                full['dq'][:, cls_row] = out['dq_cls'].emu
        rq = ABO._rb if self.rnd else (lambda t: t)
        if plant == 'cls_kv_group_missing':
            for x in ('dk', 'dv'):
                full[x][:, cls_row] = rq(rq(out['partials'][x])[:, :-1].sum(1))
        if plant == 'cls_dq_first_group_only':
            full['dq'][:, cls_row] = rq(rq(out['partials']['dq'])[:, 0])
        if cls_pass:
            hs = lambda t: t.transpose(1, 2).reshape(N * HEADS, -1, HD)                # noqa: E731
            c = ABO._core(hs(q[:, cls_row:cls_row + 1]), hs(k), hs(v), hs(d4[:, cls_row:cls_row + 1]), 0.125, False)
            back = lambda t: t.reshape(N, HEADS, -1, HD).transpose(1, 2)               # noqa: E731
            full['dq'][:, cls_row] = rq(back(c['dq'])[:, 0])
            full['dk'], full['dv'] = rq(full['dk'] + back(c['dk'])), rq(full['dv'] + back(c['dv']))
        return torch.cat([full[x].reshape(N, L, D) for x in ('dq', 'dk', 'dv')], -1).to(self.dt)


def _dp(dps, i, site, dt):
    t = None if dps is None else dps[i][site]
    return None if t is None else t.to(dt).view(-1, 1, 1)


def stepped_visual(sdp, x, depth, dout, dps=None, rnd=True, plant=None, dtype=F64, arm=Arm()):
    """Result(out, G, grads, F) of the stepped visual tower (module docstring).  x (N, 3, 16, 224, 224): tower_block_oracle.frontend's values."""
    R = _Run(sdp, rnd, plant, dtype, arm)
    sd, N = R.sd, x.shape[0]
    xin = R.r16(x.to(dtype))
    C, T, H, W = xin.shape[1:]
    patches = xin.reshape(N, C, T // 2, 2, H // 16, 16, W // 16, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N, VP, C * 2 * 256)
    X = torch.cat([sd[V + '.cls_token'].expand(N, 1, -1), R.lin(patches, V + '.patch_embed_3d.proj')], 1) + SC.vis_pos_table(sd, V)
    blocks = []
    for i in range(depth):
        p = f'{V}.blocks.{i}'
        s = dict(x=X)
        s['ht'] = R.r16(R.ln(X, p + '.norm3', EPS_V))
        s['qkvt'] = R.r16(R.lin(s['ht'], p + '.timeattn.qkv'))
        s['attt'] = R.r16(R.st.attention(s['qkvt'], 'time', None, False, False)).to(dtype)
        X = s['xt'] = X + R.lin(s['attt'], p + '.timeattn.proj')
        s['hs'] = R.r16(R.ln(X, p + '.norm1', EPS_V))
        s['qkvs'] = R.r16(R.lin(s['hs'], p + '.attn.qkv'))
        s['atts'] = R.r16(R.st.attention(s['qkvs'], 'space', None, True, True)).to(dtype)
        br, dp = R.lin(s['atts'], p + '.attn.proj'), _dp(dps, i, 0, dtype)
        X = s['xs'] = X + (br if dp is None else br * dp)
        X, s['mlp'] = R.mlp_fwd(X, p + '.norm2', EPS_V, p + '.mlp.fc1', p + '.mlp.fc2', _dp(dps, i, 1, dtype))
        blocks.append(s)
    xf = R.ln(X[:, 1:], V + '.norm', EPS_V).reshape(N * FRAMES, NTOK, D)
    Z = torch.cat([sd[VAGG + '.cls_token'].expand(N * FRAMES, 1, D), xf], 1)
    out, agg = R.agg_fwd(Z, VAGG)
    # ---- backward
    dZ = R.agg_bwd(dout, agg, VAGG)
    dx = torch.cat([torch.zeros(N, 1, D, dtype=dtype, device=x.device), R.ln_bwd(X[:, 1:], V + '.norm', dZ[:, 1:].reshape(N, VP, D), EPS_V)], 1)
    G = {}
    fused = arm.fused_attn
    for i in reversed(range(depth)):
        p, s = f'{V}.blocks.{i}', blocks[i]
        last = plant is not None and i == depth - 1
        dpm, dps_ = _dp(dps, i, 1, dtype), _dp(dps, i, 0, dtype)
        dy_b = R.head(dx, dpm, p + '.mlp.fc2.bias', unscaled_bias=last and plant == 'bias_unscaled')
        G[(i, 'mlp')] = R.mlp_bwd(s['mlp'], dy_b, p + '.norm2', EPS_V, p + '.mlp.fc1', p + '.mlp.fc2')
        dx_old, dx = dx, dx + G[(i, 'mlp')]
        for kind, key, att, ln, x_in, dp in (('space', 's', 'attn', 'norm1', s['xt'], dps_), ('time', 't', 'timeattn', 'norm3', s['x'], None)):
            sp = last and kind == 'space'
            dy_b = R.head(dx_old if sp and plant == 'stale_branch_head' else dx, dpm if sp and plant == 'dp_wrong_site' else dp, f'{p}.{att}.proj.bias')
            dO_b = R.lin_bwd(f'{p}.{att}.proj', dy_b, s['att' + key], bias=False)
            geo = (196, 1, 1, 196, 8, 0) if kind == 'time' else (8, 1, 196, 1, 196, 0)
            dqkv = R.grouped_bwd(s['qkv' + key], dO_b, geo, clsq=fused and arm.cls_in_group, round_mid=kind == 'space' or not fused,
                                 fwd_packs_p=kind == 'space', cls_pass=not (fused and arm.cls_in_group),
                                 plant={'cls_kv_group_missing_time': 'cls_kv_group_missing'}.get(plant, plant) if (sp and plant == 'cls_kv_group_missing') or
                                 (last and kind == 'time' and plant in ('cls_dq_first_group_only', 'cls_kv_group_missing_time')) else None)
            dh = R.lin_bwd(f'{p}.{att}.qkv', dqkv, s['h' + key], drop_chunk=sp and plant == 'wgrad_last_chunk_dropped')
            G[(i, kind)] = R.ln_bwd(x_in, f'{p}.{ln}', dh, EPS_V)
            dx = dx + G[(i, kind)]
    gtab, atab = dx.sum(0), dx.abs().sum(0)
    body, abody = gtab[1:].view(FRAMES, NTOK, D), atab[1:].view(FRAMES, NTOK, D)
    R.put(V + '.cls_token', gtab[0], U32 * N * atab[0])
    R.put(V + '.pos_embed', torch.cat([gtab[:1], body.sum(0)], 0), U32 * (N + FRAMES) * torch.cat([atab[:1], abody.sum(0)], 0))
    R.put(V + '.temp_embed', body.sum(1), U32 * (N + NTOK) * abody.sum(1))
    R.lin_bwd(V + '.patch_embed_3d.proj', R.r16(dx[:, 1:]), patches, need_dx=False)
    return Result(out, G, R.g, R.F)


def stepped_audio(sdp, spec, depth, dout, rnd=True, plant=None, dtype=F64, arm=Arm()):
    """Result(out, G, grads, F) of the stepped AST (module docstring).  spec (N, 128, 66)."""
    R = _Run(sdp, rnd, plant, dtype, arm)
    sd, N = R.sd, spec.shape[0]
    e = A + '.ast.embeddings'
    patches = R.r16(spec.to(dtype).unfold(1, 16, 10).unfold(2, 16, 10).reshape(N, AP, 256))
    X = torch.cat([sd[e + '.cls_token'].expand(N, 1, -1), sd[e + '.distillation_token'].expand(N, 1, -1), R.lin(patches, e + '.patch_embeddings.projection')], 1)
    X = X + sd[e + '.position_embeddings'][:, :AL]
    layers = []
    qkvn = ('query', 'key', 'value')
    for i in range(depth):
        p = f'{A}.ast.encoder.layer.{i}'
        s = dict(x=X)
        s['h1'] = R.r16(R.ln(X, p + '.layernorm_before', EPS_A))
        s['qkv'] = torch.cat([R.r16(R.lin(s['h1'], f'{p}.attention.attention.{nm}')) for nm in qkvn], -1)
        hs = lambda t: t.reshape(N, AL, HEADS, HD).transpose(1, 2)                      # noqa: E731
        q, k, v = hs(s['qkv'][..., :D]) * 0.125, hs(s['qkv'][..., D:2 * D]), hs(s['qkv'][..., 2 * D:])
        s['att'] = R.r16(R.st.softmax_pv(q, k, v, None, True).to(dtype).transpose(1, 2).reshape(N, AL, D))
        X = s['x2'] = X + R.lin(s['att'], p + '.attention.output.dense')
        X, s['mlp'] = R.mlp_fwd(X, p + '.layernorm_after', EPS_A, p + '.intermediate.dense', p + '.output.dense')
        layers.append(s)
    xf = R.ln(X[:, 2:], A + '.ast.layernorm', EPS_A)
    per_t = xf.reshape(N, ANF, ANT, D).transpose(1, 2).reshape(N * ANT, ANF, D)
    out, agg = R.agg_fwd(torch.cat([sd[AAGG + '.cls_token'].expand(N * ANT, 1, D), per_t], 1), AAGG)
    # ---- backward
    dZ = R.agg_bwd(dout, agg, AAGG)
    dxf = dZ[:, 1:].reshape(N, ANT, ANF, D).transpose(1, 2).reshape(N, AP, D)
    dx = torch.cat([torch.zeros(N, 2, D, dtype=dtype, device=spec.device), R.ln_bwd(X[:, 2:], A + '.ast.layernorm', dxf, EPS_A)], 1)
    G = {}
    for i in reversed(range(depth)):
        p, s = f'{A}.ast.encoder.layer.{i}', layers[i]
        dy_b = R.head(dx, None, p + '.output.dense.bias')
        G[(i, 'mlp')] = R.mlp_bwd(s['mlp'], dy_b, p + '.layernorm_after', EPS_A, p + '.intermediate.dense', p + '.output.dense')
        dx = dx + G[(i, 'mlp')]
        dy_b = R.head(dx, None, p + '.attention.output.dense.bias')
        dO_b = R.lin_bwd(p + '.attention.output.dense', dy_b, s['att'], bias=False)
        dqkv = R.grouped_bwd(s['qkv'], dO_b, (1, 0, 0, 1, AL, -1), clsq=False, round_mid=True, fwd_packs_p=False, cls_pass=False)
        dh = sum(R.lin_bwd(f'{p}.attention.attention.{nm}', dqkv[..., j * D:(j + 1) * D], s['h1'], round_dx=False) for j, nm in enumerate(qkvn))
        G[(i, 'attn')] = R.ln_bwd(s['x'], p + '.layernorm_before', dh, EPS_A)
        dx = dx + G[(i, 'attn')]
    gtab, atab = dx.sum(0), dx.abs().sum(0)
    gpos, fpos = torch.zeros_like(sd[e + '.position_embeddings']), torch.zeros_like(sd[e + '.position_embeddings'])
    gpos[0, :AL], fpos[0, :AL] = gtab, U32 * N * atab
    R.put(e + '.position_embeddings', gpos, fpos)
    R.put(e + '.cls_token', gtab[0], U32 * N * atab[0])
    R.put(e + '.distillation_token', gtab[1], U32 * N * atab[1])
    R.lin_bwd(e + '.patch_embeddings.projection', R.r16(dx[:, 2:]), patches, need_dx=False)
    return Result(out, G, R.g, R.F)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ratio(e, bar):
    """e / bar; where the bar is zero the quantity must be exact: 0 if it is, inf if not."""
    return torch.where(bar > 0, e / bar.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, math.inf), torch.zeros_like(e)))


def vis_classes(n, dp=None, device='cpu'):
    """name -> (n, 1569) masks: the forward oracle's CLS / side / patch classes; dp (n,): kept and dropped segments of the branch's DropPath site separately."""
    base = TB.row_classes(n, None, device)
    if dp is None:
        return base
    kept = (dp.reshape(-1) != 0).to(device).view(n, 1)
    out = {}
    for nm, m in base.items():
        for tag, seg in (('kept', kept), ('dropped', ~kept)):
            if (m & seg).any():
                out[f'{nm}_{tag}'] = m & seg
    return out


def aud_classes(n, device='cpu'):
    cls = torch.zeros(n, AL, dtype=torch.bool, device=device)
    cls[:, :2] = True
    return dict(cls=cls, patch=~cls)


def check_rows(g_eng, g_exact, g_step, classes):
    """Criterion (A): class -> (worst row err / bar, summed err / summed bar, worst per-segment class-mean err / bar); all must be <= 1."""
    err, noise = (g_eng - g_exact).norm(dim=-1), (g_step - g_exact).norm(dim=-1)
    out = {}
    for name, m in classes.items():
        e, n = err[m], noise[m]
        row = _ratio(e, MARGIN_A * torch.maximum(n, n.median())).max().item()
        tot = _ratio(e.sum(), MARGIN_A * n.sum()).item()
        cnt = m.sum(1)
        live = cnt > 0
        w = (m.to(g_eng.dtype) / cnt.clamp_min(1).unsqueeze(1)).unsqueeze(-1)
        me, mn = ((g_eng - g_exact) * w).sum(1).norm(dim=-1)[live], ((g_step - g_exact) * w).sum(1).norm(dim=-1)[live]
        out[name] = (row, tot, _ratio(me, MARGIN_A * torch.maximum(mn, mn.median())).max().item())
    return out


def noise_levels(g_exact, g_step, classes):
    """class -> rel-RMS of the stepped model's noise (report only)."""
    return {name: ((g_step - g_exact)[m].pow(2).sum().sqrt() / g_exact[m].pow(2).sum().sqrt().clamp_min(1e-300)).item() for name, m in classes.items()}


def _blocks(t):
    """(N, K) with N, K multiples of 128 -> per 128 x 128 block Frobenius norms (N / 128, K / 128)."""
    N, K = t.shape
    return t.reshape(N // 128, 128, K // 128, 128).pow(2).sum((1, 3)).sqrt()


def check_grads(g_eng, g_exact, g_step, F):
    """Criterion (G): key -> (tensor err / bar, worst 128 x 128 block err / bar or None, F share of the tensor bar); the first two must be <= 1."""
    out = {}
    for k, ge in g_exact.items():
        e, n = (g_eng[k].to(ge.dtype) - ge), (g_step[k].to(ge.dtype) - ge)
        f = F[k].to(ge.dtype).norm() if F is not None and k in F else ge.new_zeros(())
        bar = MARGIN_A * n.norm() + f
        blk = None
        if ge.dim() >= 2 and (k.endswith('.weight') or k.endswith('in_proj_weight')):
            e2, n2 = e.reshape(ge.shape[0], -1), n.reshape(ge.shape[0], -1)
            if e2.shape[0] % 128 == 0 and e2.shape[1] % 128 == 0:
                blk = _ratio(_blocks(e2), MARGIN_A * _blocks(n2)).max().item()
        out[k] = (_ratio(e.norm(), bar).item(), blk, (f / bar.clamp_min(1e-300)).item())
    return out


def worst_rows(checks):
    """(largest of the row / sum / mean ratios of a check_rows result, its class)."""
    return max((max(v), k) for k, v in checks.items())


def worst_grads(checks):
    """(largest tensor ratio, key), (largest block ratio, key) of a check_grads result."""
    t = max((v[0], k) for k, v in checks.items())
    b = max(((v[1], k) for k, v in checks.items() if v[1] is not None), default=(0.0, None))
    return t, b
