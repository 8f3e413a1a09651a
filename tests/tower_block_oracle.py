"""Float64 oracle of the visual tower's DividedSpaceTimeBlocks as the engine schedules them (tests/test_tower_blocks_gpu.py, tests/test_tower_block_oracle_cpu.py).
Pure torch, no kernel of the library: every function runs on the device its tensors live on (the GPU test runs it on the device in float64, the screen on the CPU).

Two models of one forward (frontend -> patch embedding + table -> `depth` blocks -> final norm + aggregator layer, row 0 of every frame):

  exact    oracle.synchformer_cpu's own functions (patch_embed_3d, vis_pos_table, divided_block, agg_encoder_layer_cls) in float64 on a state dict whose GEMM weights
           hold the values the engine multiplies by (prepare_sd): bf16-rounded, or - fp8 towers - the host MXFP8 quantisation (rowops_fwd_oracle.mx_quant_int, integer
           arithmetic on the bf16 bits) of the bf16-rounded weight, dequantised (gemm_oracle.mx_dequant).  No activation is rounded; the frames are the fp16 values
           of the u8 front-end.
  stepped  the same computation written out here (stepped_tower), with the activations rounded where a schedule stores them (Schedule):
             frames            bf16 (the im2col launches write bf16 patches)
             LayerNorm output  bf16; fp8: quantize_mxfp8 of that bf16 row (block scales per 32 columns) - sf_layernorm768_mxfp8, sf_gemm_mx_res_ln768 and the mixed
                               policy's sf_gemm_res_ln768 + sf_quantize_mxfp8 all store exactly this
             q | k | v         bf16 (every projection, fused or not; the side / CLS rows come from a GEMM with a bf16 output)
             softmax weights   bf16 where the launch packs its un-normalised exponentials before P V (attn_mfma_kernel and its copies in sf_qkv_space / sf_qkv_time2:
                               every space launch's patch rows; the space CLS row unless SF_CLS_FUSION=none sends it through attn_cls64_kernel; the time half only on
                               sf_qkv_time_attention2[_mx]): Schedule.pack_time, Schedule.pack_space_cls.  As in test_attention_fwd_gpu._attend: l is summed before
                               the packing, the exponentials are taken at the exact maximum
             attention output  bf16; fp8: quantize_mxfp8 of it unless the projection keeps bf16 operands ('proj' in Schedule.lin_bf16)
             GELU hidden       bf16; fp8: quantize_mxfp8 of it unless fc2 keeps bf16 operands ('fc2' in Schedule.lin_bf16)
             tail              the aggregator's folded value + output projection W_o[:, h] W_v[h] rounded to bf16 (engine.agg_cls_operands, restated here), its bf16
                               softmax weights, bf16 norm2 output and bf16 GELU hidden
           The fp32 residual stream is not rounded.  With rnd=False every rounding is the identity and stepped must equal exact to 1e-12 (the screen checks it).
           mm = c: the fp32 variant - every Linear accumulated in float32 as c chunks of K (chunk products in fp32, summed in fp32), LayerNorm, q k^T, softmax, P V and
           GELU in float32 - which measures how often fp32 arithmetic flips a rounding of the stepped model (`flip`, criterion B).

Criteria (on the block's update U_b = X_after_b - X_before_b, rows of a segment split into classes - the CLS row, the 32 side rows = patches 192 .. 195 of every frame,
the other patch rows; under a token mask kept and dropped tokens separately):
  (A) per row err(r) = ||U_engine(r) - U_exact(r)||_2 <= 1.5 max(noise(r), median of the class's noise), noise(r) = ||U_stepped(r) - U_exact(r)||_2; and the class sums.
  (A-mean) the same bar on the mean over the rows of a class, per segment (check_mean): added when the screen showed that a missing side-row bias - an error of
      0.3 % of the update, the same in every row - stays inside (A) and (B), because a perturbation of 1e-5 in front of a chain of bf16 roundings comes out of the
      block as 1e-3 (every later rounding flips with probability |delta| / ulp and each flip is a whole ulp), which is also why `flip` is half the noise.
  (B) per class rel-RMS of U_engine - U_stepped over the RMS of U_exact <= 4 flip(class), flip = the larger deviation of the two fp32 variants (mm = 2, mm = 8).
MARGIN_A = 1.5 and FACTOR_B = 4 are stated by the issue before any measurement and are not fitted.

`plant` names the defects of the screen (PLANTS): each is an error a wrong schedule branch would make, applied inside stepped_tower."""
import math
import os
import sys
from collections import namedtuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
sys.path.insert(0, os.path.dirname(_HERE))
import gemm_oracle as GO  # noqa: E402
import rowops_fwd_oracle as RO  # noqa: E402
from oracle import synchformer_cpu as SC  # noqa: E402

D, FF, L, HEADS, HD, FRAMES, NTOK = 768, 3072, 1569, 12, 64, 8, 196
EPS = SC.EPS_VIS
V = 'vfeat_extractor'
AGG = V + '.spatial_attn_agg'
BIG = ('timeattn.qkv', 'timeattn.proj', 'attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')
MARGIN_A, FACTOR_B = 1.5, 4.0
F64 = torch.float64

Schedule = namedtuple('Schedule', 'prec lin_bf16 pack_time pack_space_cls', defaults=(frozenset(), True, True))
PLANTS = ('side_no_bias', 'cls_keys_wrong_segment', 'scale_byte', 'gamma_swap', 'skip_requant', 'stale_hidden')


def rb(x):
    """-> nearest bf16, in the dtype of x."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def mx_round(x):
    """quantize_mxfp8 followed by the dequantisation, on bf16 values held in float32 / float64 (rows.., K), K % 32 == 0: scale 2^(floor(log2 amax) - 8) per 32-block,
    byte clamped to 1 .. 254, elements saturated to +-448 and rounded to nearest-even e4m3 (3 mantissa bits, normals from 2^-6, subnormal step 2^-9).  frexp and
    ldexp only: exact on any device.  The screen holds it to rowops_fwd_oracle.mx_quant_int bit for bit."""
    shp = x.shape
    b = x.reshape(-1, shp[-1] // 32, 32).to(F64)
    amax = b.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -126)
    e = (torch.frexp(amax)[1] - 1 - 8).clamp(-126, 127)
    s = torch.ldexp(b, -e).clamp(-448.0, 448.0)
    p = (torch.frexp(s.abs().clamp_min(2.0 ** -40))[1] - 1).clamp_min(-6) - 3
    q = torch.ldexp(torch.round(torch.ldexp(s, -p)), p).clamp(-448.0, 448.0)
    return torch.ldexp(q, e).reshape(shp).to(x.dtype)


def side_rows():
    """Rows of a segment that the fused launches take from the side GEMM, without the CLS row: patches 192 .. 195 of every frame."""
    return (1 + torch.arange(FRAMES).view(-1, 1) * NTOK + 192 + torch.arange(4).view(1, -1)).reshape(-1)


def row_classes(n, tok_keep=None, device='cpu'):
    """name -> (n, 1569) bool masks; empty classes are left out."""
    cls = torch.zeros(n, L, dtype=torch.bool, device=device)
    cls[:, 0] = True
    side = torch.zeros_like(cls)
    side[:, side_rows().to(device)] = True
    patch = ~(cls | side)
    if tok_keep is None:
        return dict(cls=cls, side=side, patch=patch)
    k = tok_keep.to(device)
    out = dict(cls=cls, side_kept=side & k, side_dropped=side & ~k, patch_kept=patch & k, patch_dropped=patch & ~k)
    return {a: m for a, m in out.items() if m.any()}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------------
def frontend(u8):
    """(B, S, 16, 3, 224, 224) uint8 -> (B S, 3, 16, 224, 224) float64: the fp16 values of the u8 front-end (oracle.synchformer_cpu.rgb_frontend)."""
    B, S = u8.shape[:2]
    return SC.rgb_frontend(u8).reshape(B * S, *u8.shape[2:]).permute(0, 2, 1, 3, 4).to(F64)


def token_keep(sd, vis_mask):
    """(B, S, 16, 3, 224, 224) bool content mask -> (B S, 1569) bool token flags, CLS kept (motionformer_segments' own lines)."""
    B, S = vis_mask.shape[:2]
    m = vis_mask.reshape(B * S, *vis_mask.shape[2:]).permute(0, 2, 1, 3, 4).bool()
    w = sd[V + '.patch_embed_3d.proj.weight']
    N, C, T, H, W = m.shape
    pk = m.reshape(N, C, T // 2, 2, H // 16, 16, W // 16, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N, -1, C * 2 * 256)
    tk = SC.token_mask_from_content(pk, w[0].reshape(-1).to(m.device))
    return torch.cat([torch.ones(N, 1, dtype=torch.bool, device=m.device), tk], 1)


def mx_weight(w):
    """fp32 weight (N, K) -> (bytes (N, K) uint8, scale bytes (N, K / 32) uint8) of the bf16-rounded weight, on the host."""
    return RO.mx_quant_int(w.detach().cpu().to(torch.bfloat16))


def prepare_sd(sd, sch, device='cpu'):
    """The float64 state dict of both models for one schedule family: patch embedding, aggregator and (bf16 towers, or the mixed policy's Linears) block weights
    bf16-rounded; fp8 towers: the six big Linears of every block MXFP8-quantised on the host and dequantised.  Everything else is the fp32 value."""
    out = {}
    bf = lambda t: t.detach().to(torch.bfloat16).to(F64)                              # noqa: E731
    for k, t in sd.items():
        if not k.startswith(V + '.'):
            continue
        if k.endswith('.weight') and t.dim() >= 2 or k.endswith('in_proj_weight'):
            name = k[:-len('.weight')]
            big = name.startswith(V + '.blocks.') and name.split('.', 3)[3] in BIG
            kind = name.rsplit('.', 1)[-1]
            if big and sch.prec == 'mx' and kind not in sch.lin_bf16:
                out[k] = GO.mx_dequant(*mx_weight(t))
            else:
                out[k] = bf(t)
        else:
            out[k] = t.detach().to(F64)
    return {k: t.to(device) for k, t in out.items()}


def folded_agg(sdp):
    """engine.agg_cls_operands restated: (u (12, 768), c (12,), w_vo (12, 768, 768) = W_o[:, h] W_v[h], b_vo (768,)) in float64 from the prepared weights."""
    x = sdp[AGG + '.cls_token'].reshape(-1)
    ln = lambda t, n: (t - t.mean(-1, keepdim=True)) / torch.sqrt(t.var(-1, unbiased=False, keepdim=True) + EPS) * sdp[n + '.weight'] + sdp[n + '.bias']   # noqa: E731
    zn_cls = ln(x, AGG + '.norm1')
    w_in, b_in, w_o, b_o = sdp[AGG + '.self_attn.in_proj_weight'], sdp[AGG + '.self_attn.in_proj_bias'], sdp[AGG + '.self_attn.out_proj.weight'], sdp[AGG + '.self_attn.out_proj.bias']
    return zn_cls, w_in, b_in, w_o, b_o, x


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def exact_tower(sdp, x, depth, tok_keep=None):
    """dict(X0, X = [after block 0, ..], feats (N, 8, 768)) through oracle.synchformer_cpu in float64."""
    N = x.shape[0]
    tok = SC.patch_embed_3d(x, sdp[V + '.patch_embed_3d.proj.weight'], sdp[V + '.patch_embed_3d.proj.bias'])
    X = torch.cat([sdp[V + '.cls_token'].expand(N, 1, -1), tok], 1) + SC.vis_pos_table(sdp, V)
    out = dict(X0=X, X=[])
    for i in range(depth):
        X = SC.divided_block(X, sdp, f'{V}.blocks.{i}', tok_keep)
        out['X'].append(X)
    xf = SC._ln(X[:, 1:], sdp, V + '.norm', EPS)
    keep = None if tok_keep is None else tok_keep[:, 1:].reshape(N * FRAMES, -1)
    out['feats'] = SC.agg_encoder_layer_cls(xf.reshape(N * FRAMES, NTOK, -1), sdp, AGG, keep=keep).reshape(N, FRAMES, -1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stepped
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _Step:
    def __init__(self, sdp, sch, rnd, mm, plant):
        self.sd, self.sch, self.rnd, self.mm, self.plant = sdp, sch, rnd, mm, plant
        self.wt = torch.float32 if mm else F64

    def r16(self, x):
        return rb(x) if self.rnd else x

    def r8(self, x, lin=None):
        """The operand of an MX GEMM: quantize_mxfp8 of the bf16 values (identity on the bf16 towers, and for a Linear the mixed policy keeps on bf16 operands)."""
        if not self.rnd or self.sch.prec != 'mx' or lin in self.sch.lin_bf16:
            return x
        return mx_round(x)

    def lin(self, a, name, bias=True):
        w, b = self.sd[name + '.weight'], self.sd[name + '.bias'] if bias else None
        w = w.reshape(w.shape[0], -1)
        if not self.mm:
            y = a @ w.t()
        else:
            a32, w32, K = a.to(torch.float32), w.to(torch.float32), w.shape[1]
            step = K // self.mm
            y = None
            for c in range(self.mm):
                part = a32[..., c * step:(c + 1) * step] @ w32[:, c * step:(c + 1) * step].t()
                y = part if y is None else y + part
            if b is not None:
                y = y + b.to(torch.float32)
            return y.to(F64)
        return y if b is None else y + b

    def ln(self, x, name):
        g, b = self.sd[name + '.weight'], self.sd[name + '.bias']
        if self.mm:
            return torch.nn.functional.layer_norm(x.to(torch.float32), (D,), g.to(torch.float32), b.to(torch.float32), EPS).to(F64)
        return torch.nn.functional.layer_norm(x, (D,), g, b, EPS)

    def gelu(self, x):
        if self.mm:
            return torch.nn.functional.gelu(x.to(torch.float32)).to(F64)
        return GO.gelu64(x)

    def softmax_pv(self, q, k, v, mask, pack):
        """q (.., Tq, d) already scaled, k, v (.., nk, d), mask (.., 1 | Tq, nk) or None -> p v with the kernel's packing."""
        q, k, v = q.to(self.wt), k.to(self.wt), v.to(self.wt)
        s = q @ k.mT
        if mask is not None:
            s = s.masked_fill(~mask, -math.inf)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        l = e.sum(-1, keepdim=True)
        if pack and self.rnd:
            e = rb(e)
        return ((e @ v) / l).to(F64)

    def attention(self, qkv, mode, tok_keep, pack_patch, pack_cls, cls_kv_shift=0):
        """DividedAttention's softmax part on qkv (N, 1569, 2304): CLS query over all keys, patch (f, n) over [CLS; its group]."""
        N = qkv.shape[0]
        t = qkv.reshape(N, L, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
        q, k, v = t[0] * (HD ** -0.5), t[1], t[2]
        kk = None if tok_keep is None else tok_keep[:, None, None, :]
        kc, vc = (k, v) if not cls_kv_shift else (k.roll(cls_kv_shift, 0), v.roll(cls_kv_shift, 0))
        o_cls = self.softmax_pv(q[:, :, :1], kc, vc, kk, pack_cls)

        def grp(a):
            a = a[:, :, 1:].reshape(N, HEADS, FRAMES, NTOK, HD)
            return a.transpose(2, 3) if mode == 'time' else a
        qg, kg, vg = grp(q), grp(k), grp(v)
        G = qg.shape[2]
        kg = torch.cat([k[:, :, :1].unsqueeze(2).expand(N, HEADS, G, 1, HD), kg], 3)
        vg = torch.cat([v[:, :, :1].unsqueeze(2).expand(N, HEADS, G, 1, HD), vg], 3)
        gk = None
        if tok_keep is not None:
            mg = tok_keep[:, 1:].reshape(N, FRAMES, NTOK)
            mg = mg.transpose(1, 2) if mode == 'time' else mg
            gk = torch.cat([tok_keep[:, :1].unsqueeze(1).expand(N, G, 1), mg], 2)[:, None, :, None, :]
        og = self.softmax_pv(qg, kg, vg, gk, pack_patch)
        if mode == 'time':
            og = og.transpose(2, 3)
        o = torch.cat([o_cls, og.reshape(N, HEADS, FRAMES * NTOK, HD)], 2)
        return o.transpose(1, 2).reshape(N, L, D)


def stepped_tower(sdp, x, depth, sch, tok_keep=None, rnd=True, mm=None, plant=None):
    """dict(X0, X, feats) of the stepped model (module docstring).  plant: one of PLANTS, applied in the last block (scale_byte, skip_requant: fp8 schedules)."""
    assert plant is None or plant in PLANTS
    st = _Step(sdp, sch, rnd, mm, plant)
    N = x.shape[0]
    xin = st.r16(x)
    C, T, H, W = xin.shape[1:]
    p = xin.reshape(N, C, T // 2, 2, H // 16, 16, W // 16, 16).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N, FRAMES * NTOK, C * 2 * 256)
    tok = st.lin(p, V + '.patch_embed_3d.proj')
    X = torch.cat([sdp[V + '.cls_token'].expand(N, 1, -1), tok], 1) + SC.vis_pos_table(sdp, V)
    out = dict(X0=X, X=[])
    side = torch.cat([torch.zeros(1, dtype=torch.int64), side_rows()]).to(x.device)
    h_prev = None
    for i in range(depth):
        b = f'{V}.blocks.{i}'
        last = plant is not None and i == depth - 1
        # time
        y3 = st.r8(st.r16(st.ln(X, b + '.norm3')))
        a = st.attention(st.r16(st.lin(y3, b + '.timeattn.qkv')), 'time', tok_keep, sch.pack_time, sch.pack_time)
        a = st.r8(st.r16(a), 'proj')
        if last and plant == 'scale_byte':                                            # head 3, its first 32-block: scale byte + 1
            a = a.clone()
            a[..., 3 * HD:3 * HD + 32] *= 2.0
        X = X + st.lin(a, b + '.timeattn.proj')
        # space
        y1 = st.r8(st.r16(st.ln(X, b + '.norm1')))
        if last and plant == 'skip_requant':                                          # xq / xs still hold norm3's rows
            y1 = y3
        qkv = st.lin(y1, b + '.attn.qkv')
        if last and plant == 'side_no_bias':
            qkv = qkv.clone()
            qkv[:, side] -= sdp[b + '.attn.qkv.bias']
        a = st.attention(st.r16(qkv), 'space', tok_keep, True, sch.pack_space_cls, cls_kv_shift=1 if last and plant == 'cls_keys_wrong_segment' else 0)
        X = X + st.lin(st.r8(st.r16(a), 'proj'), b + '.attn.proj')
        # MLP
        n2 = b + ('.norm1' if last and plant == 'gamma_swap' else '.norm2')
        y2 = st.ln(X, b + '.norm2')
        if n2 != b + '.norm2':
            y2 = (y2 - sdp[b + '.norm2.bias']) / sdp[b + '.norm2.weight'] * sdp[n2 + '.weight'] + sdp[b + '.norm2.bias']
        h = st.r8(st.r16(st.gelu(st.lin(st.r8(st.r16(y2)), b + '.mlp.fc1'))), 'fc2')
        if last and plant == 'stale_hidden':
            assert h_prev is not None, 'stale_hidden needs two blocks'
            h = h_prev
        h_prev = h
        X = X + st.lin(h, b + '.mlp.fc2')
        out['X'].append(X)
    out['feats'] = _stepped_tail(st, X, tok_keep)
    out['feats_plain'] = _stepped_tail(_Step(sdp, sch, False, None, None), X, tok_keep)       # the stepped blocks under an unrounded tail
    return out


def _stepped_tail(st, X, tok_keep):
    """Final norm + the aggregator layer's row 0 in the engine's pooled form (sf_agg_cls_pool + the folded value / output projection), module docstring."""
    sdp, N = st.sd, X.shape[0]
    zn_cls, w_in, b_in, w_o, b_o, cls_tok = folded_agg(sdp)
    xf = st.ln(X[:, 1:], V + '.norm').reshape(N * FRAMES, NTOK, D)
    zn = torch.cat([zn_cls.expand(N * FRAMES, 1, D), st.ln(xf, AGG + '.norm1')], 1)                                    # keys: [cls; tokens]
    q = (w_in[:D] @ st.r16(zn_cls) + b_in[:D]).view(HEADS, HD)
    w_k, b_k = w_in[D:2 * D].view(HEADS, HD, D), b_in[D:2 * D].view(HEADS, HD)
    w_v, b_v = w_in[2 * D:].view(HEADS, HD, D), b_in[2 * D:]
    u = HD ** -0.5 * torch.einsum('hd,hdk->hk', q, w_k)
    c = HD ** -0.5 * (q * b_k).sum(1)
    s = torch.einsum('hk,njk->nhj', u, zn) + c.view(1, HEADS, 1)
    if tok_keep is not None:
        kk = torch.cat([torch.ones(N * FRAMES, 1, dtype=torch.bool, device=X.device), tok_keep[:, 1:].reshape(N * FRAMES, NTOK)], 1)
        s = s.masked_fill(~kk[:, None, :], -math.inf)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    l = e.sum(-1, keepdim=True)
    G = torch.einsum('nhj,njk->nhk', st.r16(e), zn) / l                                                               # pooled normalised rows per head
    w_vo = torch.stack([st.r16(w_o[:, h * HD:(h + 1) * HD] @ w_v[h]) for h in range(HEADS)])                           # (12, 768, 768)
    y = torch.einsum('hok,nhk->no', w_vo, G) + (w_o @ b_v + b_o + cls_tok)
    yn = st.r16(st.ln(y, AGG + '.norm2'))
    h = st.r16(st.gelu(st.lin(yn, AGG + '.linear1')))
    return (y + st.lin(h, AGG + '.linear2')).reshape(N, FRAMES, D)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------------------------------------------------------
def updates(t, x0=None):
    """[U_0, U_1, ..] of a tower dict (or of a list of residual streams with x0 = the stream in front of block 0)."""
    xs = [t['X0'] if x0 is None else x0] + list(t['X'] if isinstance(t, dict) else t)
    return [b - a for a, b in zip(xs[:-1], xs[1:])]


def check_a(u_eng, u_exact, u_step, classes):
    """Criterion (A): class -> (worst row err / bar, summed err / summed bar); both must be <= 1."""
    err, noise = (u_eng - u_exact).norm(dim=-1), (u_step - u_exact).norm(dim=-1)
    out = {}
    for name, m in classes.items():
        e, n = err[m], noise[m]
        bar = MARGIN_A * torch.maximum(n, n.median())
        row = torch.nan_to_num(e / bar, nan=math.inf).max().item()
        out[name] = (row, torch.nan_to_num(e.sum() / (MARGIN_A * n.sum()), nan=math.inf).item())
    return out


def check_mean(u_eng, u_exact, u_step, classes):
    """Criterion (A) on the class mean of every segment: rounding noise is independent from row to row and averages down by the square root of the class's rows, an
    error that every row of a class shares (a missing bias, a wrong gamma, a wrong scale) does not.  err = ||mean_r (U_engine - U_exact)||_2 per (segment, class),
    noise likewise from the stepped model, bar = 1.5 max(noise, median of the class's noise over the segments).  class -> worst err / bar."""
    out = {}
    for name, m in classes.items():
        cnt = m.sum(1)
        live = cnt > 0
        w = (m.to(u_eng.dtype) / cnt.clamp_min(1).unsqueeze(1)).unsqueeze(-1)
        e, n = ((u_eng - u_exact) * w).sum(1).norm(dim=-1)[live], ((u_step - u_exact) * w).sum(1).norm(dim=-1)[live]
        out[name] = torch.nan_to_num(e / (MARGIN_A * torch.maximum(n, n.median())), nan=math.inf).max().item()
    return out


def rel_rms(d, ref, m):
    return (d[m].pow(2).sum().sqrt() / ref[m].pow(2).sum().sqrt()).item()


def flip_of(u_v1, u_v2, u_step, u_exact, classes):
    """class -> (flip = the larger rel-RMS deviation of the two fp32 variants from the float64 stepped model, the ratio larger / smaller)."""
    out = {}
    for name, m in classes.items():
        a, b = rel_rms(u_v1 - u_step, u_exact, m), rel_rms(u_v2 - u_step, u_exact, m)
        out[name] = (max(a, b), max(a, b) / max(min(a, b), 1e-300))
    return out


def check_b(u_eng, u_step, u_exact, classes, flip):
    """Criterion (B): class -> rel-RMS of U_engine - U_stepped / (4 flip); must be <= 1."""
    return {name: torch.nan_to_num(torch.tensor(rel_rms(u_eng - u_step, u_exact, m) / (FACTOR_B * flip[name][0])), nan=math.inf).item() for name, m in classes.items()}


def check_feats(f_eng, f_exact, f_step):
    """Criterion (D): the (A) bar on the aggregated features, every (segment, frame) row one class: (worst row ratio, sum ratio)."""
    n = f_eng.shape[0]
    rows = {'feats': torch.ones(n, f_eng.shape[1], dtype=torch.bool, device=f_eng.device)}
    return check_a(f_eng, f_exact, f_step, rows)['feats']
