"""Tensor-level wrappers over the C ABI (one Python function per `sf_*` entry point).

torch is plumbing here: device memory (`Tensor.data_ptr()`), the current HIP stream and dtype bookkeeping.
All compute happens in libsynchformer_hip.so; there is no eager / CPU fallback - a CPU tensor raises.
Also registered as `torch.ops.synchformer.*` custom ops (see `register_torch_ops`) so the kernels are visible
to the dispatcher, as the reference's callers would expect of a PyTorch-ROCm extension.
"""
import ctypes as C
import os
import threading
from collections import namedtuple
from pathlib import Path
from typing import Optional, Sequence

import torch

from . import _lib
from .ingest import CROP as INGEST_OUT, MAX_TAPS as INGEST_MAX_TAPS     # noqa: F401  the launchers' output size and tap range, stated once (ingest.py is host-only)

SF_F32, SF_BF16, SF_F16, SF_U8 = 0, 1, 2, 3
EPI_NONE, EPI_GELU = 0, 1
_DT = {torch.float32: SF_F32, torch.bfloat16: SF_BF16, torch.float16: SF_F16, torch.uint8: SF_U8}

RowMap = Optional[Sequence[int]]   # (n12, n2, sA, s1, s2, off) or None


def rowmap(n12: int, n2: int, sA: int, s1: int, s2: int, off: int):
    return (int(n12), int(n2), int(sA), int(s1), int(s2), int(off))


def _map(m: RowMap):
    if m is None:
        return None
    assert len(m) == 6
    return (C.c_int64 * 6)(*m)


def _dev(t: torch.Tensor, name: str) -> int:
    if not t.is_cuda:
        raise RuntimeError(f'{name}: expected a HIP device tensor, got {t.device} (no CPU fallback exists)')
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, f'expected a row-major 2-D view, got {tuple(t.shape)} / {t.stride()}'
    return t.stride(0)


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, M: Optional[int] = None,
         residual: Optional[torch.Tensor] = None, gelu: bool = False, c_map: RowMap = None, r_map: RowMap = None):
    """out[cmap(m)] = act(a[m] @ w.T + bias) (+ residual[rmap(m)]).  a (>=M, K) bf16, w (N, K) bf16."""
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
    M = a.shape[0] if M is None else M
    if w.dim() == 3:                                        # k-tile-major weight (K / 64, N, 64), see ktile_major_weight()
        K, N = w.shape[0] * 64, w.shape[1]
        assert w.shape[2] == 64 and w.is_contiguous()
        w_ld = 64
    else:
        N, K = w.shape
        w_ld = _ld(w)
    assert a.shape[1] == K
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() >= N
    if residual is not None:
        assert residual.dtype == torch.float32
    rc = _lib.load().sf_gemm_bf16(
        _dev(a, 'a'), _ld(a), _dev(w, 'w'), w_ld, _dev(bias, 'bias') if bias is not None else None,
        _dev(out, 'out'), _DT[out.dtype], _ld(out), _map(c_map),
        _dev(residual, 'residual') if residual is not None else None, _ld(residual) if residual is not None else 0,
        _map(r_map), EPI_GELU if gelu else EPI_NONE, M, N, K, _stream())
    _lib.check(rc, 'sf_gemm_bf16')
    return out


def mx_scale_planes(rows: int, K: int, device) -> torch.Tensor:
    """Stage-major E8M0 scale planes for an MXFP8 operand of `rows` x K: uint8 (K / 128, rows padded to whole 256-row tiles, 4).  The padding is what
    lets sf_gemm_mxfp8 fetch a tile's scales of one stage as one contiguous KiB (one LDS-DMA piece)."""
    return torch.zeros(K // 128, ((rows + 255) // 256) * 256, 4, device=device, dtype=torch.uint8)


def quantize_mxfp8(x: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, rows: Optional[int] = None):
    """bf16 x (rows, K) -> q uint8 (rows, K) OCP e4m3 bytes + scales uint8 (K / 128, >= rows, 4): E8M0, one per 32 consecutive k, stage-major
    (scales[k // 128, r, (k // 32) % 4])."""
    assert x.dtype == torch.bfloat16 and q.dtype == torch.uint8 and scales.dtype == torch.uint8
    rows = x.shape[0] if rows is None else rows
    K = x.shape[1]
    assert q.shape[1] == K and scales.dim() == 3 and scales.shape[0] == K // 128 and scales.shape[1] >= rows and scales.shape[2] == 4 and scales.is_contiguous()
    rc = _lib.load().sf_quantize_mxfp8(_dev(x, 'x'), _ld(x), _dev(q, 'q'), _ld(q), _dev(scales, 'scales'), scales.stride(0), rows, K, _stream())
    _lib.check(rc, 'sf_quantize_mxfp8')
    return q, scales


def layernorm_mxfp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, eps: float, rows: Optional[int] = None):
    """(q, scales) = quantize_mxfp8(bf16(LayerNorm(x))) in one pass: x fp32 (rows, 768) -> q uint8 (rows, 768), scales uint8 (6, >= rows, 4)."""
    assert x.dtype == torch.float32 and x.shape[1] == 768 and q.dtype == torch.uint8 and q.shape[1] == 768
    rows = x.shape[0] if rows is None else rows
    assert scales.dtype == torch.uint8 and scales.dim() == 3 and scales.shape[0] == 6 and scales.shape[1] >= rows and scales.is_contiguous()
    rc = _lib.load().sf_layernorm768_mxfp8(_dev(x, 'x'), _ld(x), _dev(gamma, 'gamma'), _dev(beta, 'beta'), _dev(q, 'q'), _ld(q), _dev(scales, 'scales'),
                                           scales.stride(0), rows, float(eps), _stream())
    _lib.check(rc, 'sf_layernorm768_mxfp8')
    return q, scales


def gemm_mxfp8(a_q: torch.Tensor, a_s: torch.Tensor, w_q: torch.Tensor, w_s: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
               M: Optional[int] = None, residual: Optional[torch.Tensor] = None, gelu: bool = False, out_scales: Optional[torch.Tensor] = None):
    """out[m] = act(dq(a)[m] @ dq(w).T + bias) (+ residual[m]) on MXFP8 operands (see quantize_mxfp8).  With a uint8 `out` and `out_scales`
    (N / 128, >= M, 4) the result itself leaves as MXFP8."""
    assert (out.dtype == torch.uint8) == (out_scales is not None)
    assert a_q.dtype == torch.uint8 and w_q.dtype == torch.uint8 and a_s.dtype == torch.uint8 and w_s.dtype == torch.uint8
    M = a_q.shape[0] if M is None else M
    N, K = w_q.shape
    assert a_q.shape[1] == K
    assert a_s.dim() == 3 and w_s.dim() == 3 and a_s.shape[0] == K // 128 and w_s.shape[0] == K // 128 and a_s.is_contiguous() and w_s.is_contiguous()
    rc = _lib.load().sf_gemm_mxfp8(_dev(a_q, 'a_q'), _ld(a_q), _dev(a_s, 'a_s'), a_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                   _dev(bias, 'bias') if bias is not None else None, _dev(out, 'out'), _DT[out.dtype], _ld(out),
                                   _dev(out_scales, 'out_scales') if out_scales is not None else None, out_scales.stride(0) if out_scales is not None else 0,
                                   _dev(residual, 'residual') if residual is not None else None, _ld(residual) if residual is not None else 0,
                                   EPI_GELU if gelu else EPI_NONE, M, N, K, _stream())
    _lib.check(rc, 'sf_gemm_mxfp8')
    return out


def gemm_mx_res_ln(a_q: torch.Tensor, a_s: torch.Tensor, w_q: torch.Tensor, w_s: torch.Tensor, bias: Optional[torch.Tensor], x: torch.Tensor, gamma: torch.Tensor,
                   beta: torch.Tensor, y_q: torch.Tensor, y_s: torch.Tensor, eps: float, *, M: Optional[int] = None, residual: Optional[torch.Tensor] = None):
    """gemm_res_ln on MXFP8 operands with an MXFP8 output: x[m] = dq(a)[m] @ dq(w).T + bias + residual[m] (fp32, in place when residual is None or x),
    (y_q, y_s) = quantize_mxfp8(bf16(LayerNorm(x[m]) * gamma + beta)).  (y_q, y_s) may be (a_q, a_s) when K == 768."""
    assert a_q.dtype == torch.uint8 and w_q.dtype == torch.uint8 and a_s.dtype == torch.uint8 and w_s.dtype == torch.uint8 and y_q.dtype == torch.uint8 and y_s.dtype == torch.uint8
    assert x.dtype == torch.float32 and x.shape[1] == 768 and y_q.shape[1] == 768
    M = a_q.shape[0] if M is None else M
    K = a_q.shape[1]
    assert w_q.shape == (768, K)
    assert a_s.dim() == 3 and w_s.dim() == 3 and y_s.dim() == 3 and a_s.shape[0] == K // 128 and w_s.shape[0] == K // 128 and y_s.shape[0] == 6
    assert a_s.is_contiguous() and w_s.is_contiguous() and y_s.is_contiguous()
    r = x if residual is None else residual
    assert r.dtype == torch.float32
    rc = _lib.load().sf_gemm_mx_res_ln768(_dev(a_q, 'a_q'), _ld(a_q), _dev(a_s, 'a_s'), a_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                          _dev(bias, 'bias') if bias is not None else None, _dev(r, 'residual'), _ld(r), _dev(x, 'x'), _ld(x),
                                          _dev(gamma, 'gamma'), _dev(beta, 'beta'), float(eps), _dev(y_q, 'y_q'), _ld(y_q), _dev(y_s, 'y_s'), y_s.stride(0),
                                          M, K, _stream())
    _lib.check(rc, 'sf_gemm_mx_res_ln768')
    return x, y_q, y_s


def gemm_res_ln(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                y: torch.Tensor, eps: float, *, M: Optional[int] = None, residual: Optional[torch.Tensor] = None, period: Optional[int] = None):
    """x[m] = a[m] @ w.T + bias + residual[m] (fp32, in place when residual is None or x), y[m] = LayerNorm(x[m]) * gamma + beta (bf16).
    a (>= M, K) bf16, w (768, K) bf16; y may be the buffer `a` lives in (each 128-row tile reads its A rows before it writes them).
    With `period`, `residual` is a table of that many rows and row m adds residual[m % period] (sf_gemm_res_ln768_periodic)."""
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dtype == torch.float32 and y.dtype == torch.bfloat16
    K = a.shape[1]
    if w.dim() == 3:                                        # k-step-major weight (K / 32, 768, 32), see kmajor_weight()
        assert w.shape == (K // 32, 768, 32) and w.is_contiguous()
        w_ptr, ldw = _dev(w, 'w'), 32
    else:
        assert w.shape == (768, K)
        w_ptr, ldw = _dev(w, 'w'), _ld(w)
    assert x.shape[1] == 768 and y.shape[1] == 768
    M = a.shape[0] if M is None else M
    r = x if residual is None else residual
    assert r.dtype == torch.float32
    if period is not None:
        assert residual is not None and residual.shape[0] >= period and residual.shape[1] == 768 and x.shape[0] >= M and y.shape[0] >= M
        rc = _lib.load().sf_gemm_res_ln768_periodic(_dev(a, 'a'), _ld(a), w_ptr, ldw, _dev(bias, 'bias') if bias is not None else None,
                                                    _dev(r, 'residual'), _ld(r), int(period), _dev(x, 'x'), _ld(x), _dev(gamma, 'gamma'), _dev(beta, 'beta'),
                                                    float(eps), _dev(y, 'y'), _ld(y), M, K, _stream())
        _lib.check(rc, 'sf_gemm_res_ln768_periodic')
        return x, y
    rc = _lib.load().sf_gemm_res_ln768(_dev(a, 'a'), _ld(a), w_ptr, ldw, _dev(bias, 'bias') if bias is not None else None,
                                       _dev(r, 'residual'), _ld(r), _dev(x, 'x'), _ld(x), _dev(gamma, 'gamma'), _dev(beta, 'beta'), float(eps),
                                       _dev(y, 'y'), _ld(y), M, K, _stream())
    _lib.check(rc, 'sf_gemm_res_ln768')
    return x, y


def ktile_major_weight(w: torch.Tensor) -> torch.Tensor:
    """(N, K) bf16 Linear weight -> (K / 64, N, 64) for the persistent 256 x 256 x 64 kernel of sf_gemm_bf16 (contiguous 32 KiB W tile per k-tile)."""
    N, K = w.shape
    return w.view(N, K // 64, 64).permute(1, 0, 2).contiguous()


def kmajor_weight(w: torch.Tensor) -> torch.Tensor:
    """(768, K) bf16 Linear weight -> (K / 32, 768, 32): the layout sf_gemm_res_ln768 streams fastest (one contiguous 48 KiB slice per 32-deep k-step
    instead of 768 half cache lines 2 K bytes apart).  Pure data movement, done once at weight-preparation time."""
    N, K = w.shape
    return w.view(N, K // 32, 32).permute(1, 0, 2).contiguous()


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, eps: float, *,
              rows: Optional[int] = None, in_map: RowMap = None, out_map: RowMap = None, accumulate: bool = False):
    assert x.dtype == torch.float32 and x.shape[1] == 768 and out.shape[1] == 768
    rows = x.shape[0] if rows is None else rows
    rc = _lib.load().sf_layernorm768(_dev(x, 'x'), _ld(x), _map(in_map), _dev(gamma, 'gamma'), _dev(beta, 'beta'),
                                     _dev(out, 'out'), _DT[out.dtype], _ld(out), _map(out_map), int(accumulate), rows,
                                     float(eps), _stream())
    _lib.check(rc, 'sf_layernorm768')
    return out


def broadcast_rows(dst: torch.Tensor, table: torch.Tensor, n_seq: int, dst_seq_rows: int):
    assert dst.dtype == torch.float32 and table.dtype == torch.float32 and table.shape[1] == 768 and table.is_contiguous()
    rc = _lib.load().sf_broadcast_rows768(_dev(dst, 'dst'), _ld(dst), dst_seq_rows, _dev(table, 'table'), table.shape[0],
                                          n_seq, _stream())
    _lib.check(rc, 'sf_broadcast_rows768')
    return dst


def gather_rows(x: torch.Tensor, out: torch.Tensor, rows: int, in_map: RowMap = None):
    assert x.dtype == torch.float32 and x.shape[1] == 768 and out.shape[1] == 768
    rc = _lib.load().sf_gather_rows768(_dev(x, 'x'), _ld(x), _map(in_map), _dev(out, 'out'), _DT[out.dtype], _ld(out), rows,
                                       _stream())
    _lib.check(rc, 'sf_gather_rows768')
    return out


def im2col_video(vid: torch.Tensor, out: torch.Tensor):
    """vid (n_seg, 16, 3, 224, 224) contiguous of u8/f16/bf16/f32 -> out bf16 (n_seg*1568, 1536)."""
    assert vid.is_contiguous() and tuple(vid.shape[1:]) == (16, 3, 224, 224), tuple(vid.shape)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[1] == 1536
    rc = _lib.load().sf_im2col_video(_dev(vid, 'vid'), _DT[vid.dtype], _dev(out, 'out'), vid.shape[0], _stream())
    _lib.check(rc, 'sf_im2col_video')
    return out


def im2col_video_clips(vid: torch.Tensor, out: torch.Tensor, frame0: int, seg_stride: int, n_seg: int):
    """vid (n_clips, T, 3, 224, 224) u8|f16|bf16|f32 -> out bf16 (n_clips*n_seg*1568, 1536): segment (clip, s) = frames
    [frame0 + s*seg_stride, +16) of the clip, read in place (GenerateMultipleSegments on the device, dataset/transforms.py:450-451)."""
    assert vid.is_contiguous() and vid.dim() == 5 and tuple(vid.shape[2:]) == (3, 224, 224)
    rc = _lib.load().sf_im2col_video_clips(_dev(vid, 'vid'), _DT[vid.dtype], vid.shape[0], vid.shape[1], frame0, seg_stride, n_seg,
                                           _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_im2col_video_clips')
    return out


def im2col_video_tokens(vid: torch.Tensor, out: torch.Tensor, frame0: int = 0, seg_stride: int = 0, n_seg: int = 1):
    """im2col_video / im2col_video_clips into the TOKEN layout: out bf16 (segments * 1569, 1536), every segment's row 0 zero, its patches at rows 1 .. 1568."""
    assert vid.is_contiguous() and vid.dim() == 5 and tuple(vid.shape[2:]) == (3, 224, 224)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[1] == 1536 and out.shape[0] >= vid.shape[0] * n_seg * 1569
    rc = _lib.load().sf_im2col_video_tokens(_dev(vid, 'vid'), _DT[vid.dtype], vid.shape[0], vid.shape[1], frame0, seg_stride, n_seg, _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_im2col_video_tokens')
    return out


def im2col_video_crops(vid: torch.Tensor, table: torch.Tensor, out: torch.Tensor, seg_stride: int, n_seg: int, tokens: bool = True):
    """Uncropped uint8 clips vid (n_clips, T, 3, H, W), H, W >= 224, and a device int32 table (n_clips, >= 4) of rows (frame0, y0, x0, flip) ->
    out bf16: segment (clip, s) = frames frame0 + s*seg_stride .. +16 of the clip, cropped at (y0, x0) to 224 x 224 and mirrored along W when
    flip != 0.  tokens=True: the layout of im2col_video_tokens (segments * 1569 rows); False: that of im2col_video_clips (segments * 1568).
    The table is read on the device only (no host sync); rows are clamped into the clip there, validated on the host by synchformer_amd.augment."""
    assert vid.is_contiguous() and vid.dim() == 5 and vid.dtype == torch.uint8 and vid.shape[2] == 3, (vid.dtype, tuple(vid.shape))
    assert table.is_cuda and table.dtype == torch.int32 and table.dim() == 2 and table.shape[0] == vid.shape[0] and table.stride(1) == 1, \
        (table.dtype, tuple(table.shape))
    tok_rows = 1569 if tokens else 1568
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[1] == 1536 and out.shape[0] >= vid.shape[0] * n_seg * tok_rows
    rc = _lib.load().sf_im2col_video_crops(_dev(vid, 'vid'), vid.shape[0], vid.shape[1], vid.shape[3], vid.shape[4], _dev(table, 'table'), table.stride(0),
                                           seg_stride, n_seg, _dev(out, 'out'), tok_rows, _stream())
    _lib.check(rc, 'sf_im2col_video_crops')
    return out


def mel_frontend_starts(mel, wave: torch.Tensor, sample0: torch.Tensor, seg_stride: int, n_seg: int, n_samples: int) -> torch.Tensor:
    """wave fp32 (B, clip_samples) + int64 device sample0 (B,) -> log-mel (B, n_seg, 1, n_mels, pad_to) of the segments [sample0[b] + s*seg_stride,
    +n_samples) of every clip, with the tables and workspace of `mel` (a frontend.MelFrontend).  Output equals sf_mel_frontend on the materialised
    segments; sample0 is read on the device only (clamped into the clip there; synchformer_amd.augment validates it on the host)."""
    w = wave.to(torch.float32).contiguous()
    assert w.dim() == 2 and sample0.is_cuda and sample0.dtype == torch.int64 and sample0.is_contiguous() and sample0.numel() == w.shape[0], \
        (tuple(w.shape), sample0.dtype, tuple(sample0.shape))
    B, clip = w.shape
    frames = min(n_samples // mel.hop + 1, mel.pad_to)
    need = B * n_seg * frames * 513
    if mel._ws is None or mel._ws.numel() < need:
        mel._ws = torch.empty(need, device=mel.dev, dtype=torch.float32)
    out = torch.empty(B * n_seg, mel.n_mels, mel.pad_to, device=mel.dev, dtype=torch.float32)
    rc = _lib.load().sf_mel_frontend_starts(_dev(w, 'wave'), B, clip, _dev(sample0, 'sample0'), seg_stride, n_seg, n_samples, mel.hop, mel.tw_cos.data_ptr(),
                                            mel.tw_sin.data_ptr(), mel.fb.data_ptr(), mel.fb_lo.data_ptr(), mel.fb_hi.data_ptr(), mel.n_mels,
                                            mel._ws.data_ptr(), out.data_ptr(), mel.pad_to, mel.mean, mel.std, _stream())
    _lib.check(rc, 'sf_mel_frontend_starts')
    return out.reshape(B, n_seg, 1, mel.n_mels, mel.pad_to)


from .augment import S1_CLIP_COLS, S1_SEG_COLS     # noqa: E402  the table layouts of include/synchformer_hip.h (SF_S1_CLIP_COLS, SF_S1_SEG_COLS)


def _stage1_tables(clip_table: torch.Tensor, seg_table: torch.Tensor, n_clips: int, n_seg: int):
    assert clip_table.is_cuda and clip_table.dtype == torch.int32 and clip_table.dim() == 2 and clip_table.shape[0] == n_clips and \
        clip_table.shape[1] >= S1_CLIP_COLS and clip_table.stride(1) == 1, (clip_table.dtype, tuple(clip_table.shape))
    assert seg_table.is_cuda and seg_table.dtype == torch.int32 and seg_table.dim() == 2 and seg_table.shape[0] == n_clips * n_seg and \
        seg_table.shape[1] >= S1_SEG_COLS and seg_table.stride(1) == 1, (seg_table.dtype, tuple(seg_table.shape))


def stage1_video_augment(vid: torch.Tensor, clip_table: torch.Tensor, seg_table: torch.Tensor, out: torch.Tensor, frame_sums: torch.Tensor,
                         seg_stride: int, n_seg: int):
    """Uncropped uint8 clips vid (n_clips, T, 3, H, W), H, W >= 224, and the two device int32 tables of a synchformer_amd.augment.Stage1Batch ->
    out uint8 (n_clips * n_seg, 16, 3, 224, 224): the Stage-1 train transforms on the device (crop or 192 -> 224 upscale, segmenting, colour
    jitter in the drawn order, gray, flip; include/synchformer_hip.h has the tables and the arithmetic).  frame_sums: int32 workspace of
    n_clips * n_seg * 16.  The tables are read on the device only (no host sync); entries are clamped into the clip there, validated on the host."""
    assert vid.is_contiguous() and vid.dim() == 5 and vid.dtype == torch.uint8 and vid.shape[2] == 3, (vid.dtype, tuple(vid.shape))
    n = vid.shape[0] * n_seg
    _stage1_tables(clip_table, seg_table, vid.shape[0], n_seg)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * 16 * 3 * 224 * 224, (out.dtype, tuple(out.shape))
    assert frame_sums.dtype == torch.int32 and frame_sums.is_contiguous() and frame_sums.numel() >= n * 16
    rc = _lib.load().sf_stage1_video_augment(_dev(vid, 'vid'), vid.shape[0], vid.shape[1], vid.shape[3], vid.shape[4], _dev(clip_table, 'clip_table'),
                                             clip_table.stride(0), _dev(seg_table, 'seg_table'), seg_table.stride(0), seg_stride, n_seg,
                                             _dev(frame_sums, 'frame_sums'), _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_stage1_video_augment')
    return out


def stage1_audio_augment(wave: torch.Tensor, clip_table: torch.Tensor, seg_table: torch.Tensor, out: torch.Tensor, seg_stride: int, n_seg: int,
                         lowpass: Sequence[float], noise_amp: float = 0.01):
    """fp32 wave (n_clips, clip_samples) + the two device tables -> out fp32 (n_clips * n_seg, n_samples): the windows [sample0 + s*seg_stride,
    +n_samples) of every clip, then per segment volume, lowpass biquad (`lowpass` = b0, b1, b2, a1, a2 already divided by a0) and Gaussian
    noise as the segment's flags say (include/synchformer_hip.h)."""
    assert wave.is_contiguous() and wave.dim() == 2 and wave.dtype == torch.float32, (wave.dtype, tuple(wave.shape))
    _stage1_tables(clip_table, seg_table, wave.shape[0], n_seg)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == wave.shape[0] * n_seg, (out.dtype, tuple(out.shape))
    assert len(lowpass) == 5
    rc = _lib.load().sf_stage1_audio_augment(_dev(wave, 'wave'), wave.shape[0], wave.shape[1], _dev(clip_table, 'clip_table'), clip_table.stride(0),
                                             _dev(seg_table, 'seg_table'), seg_table.stride(0), seg_stride, n_seg, out.shape[1],
                                             *[float(c) for c in lowpass], float(noise_amp), _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_stage1_audio_augment')
    return out


def im2col_spec(spec: torch.Tensor, out: torch.Tensor):
    """spec fp32 (n_seg, F, Ta) contiguous -> out bf16 (n_seg*nf*nt, 256)."""
    assert spec.is_contiguous() and spec.dtype == torch.float32 and spec.dim() == 3
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[1] == 256
    rc = _lib.load().sf_im2col_spec(_dev(spec, 'spec'), _dev(out, 'out'), spec.shape[0], spec.shape[1], spec.shape[2],
                                    _stream())
    _lib.check(rc, 'sf_im2col_spec')
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, n_seq: int, seq_rows: int,
              n_groups: int, row0: int, group_stride: int, tok_stride: int, n_tok: int, cls_row: int, heads: int,
              head_dim: int, scale: float, key_keep: Optional[torch.Tensor] = None):
    """q/k/v: column-slice views (rows, heads*head_dim) of a packed bf16 projection; see include/synchformer_hip.h.
    key_keep: optional uint8 (rows,) token mask, 0 = that K/V row is masked out for every query."""
    assert q.dtype == k.dtype == v.dtype == out.dtype == torch.bfloat16
    assert _ld(q) == _ld(k) == _ld(v)
    if key_keep is None:
        rc = _lib.load().sf_attention(_dev(q, 'q'), _dev(k, 'k'), _dev(v, 'v'), _ld(q), _dev(out, 'out'), _ld(out), n_seq,
                                      seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim,
                                      float(scale), _stream())
    else:
        assert key_keep.dtype == torch.uint8 and key_keep.is_contiguous()
        rc = _lib.load().sf_attention_masked(_dev(q, 'q'), _dev(k, 'k'), _dev(v, 'v'), _ld(q), _dev(out, 'out'), _ld(out), n_seq,
                                             seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim,
                                             float(scale), _dev(key_keep, 'key_keep'), _stream())
    _lib.check(rc, 'sf_attention')
    return out


def attention_cls_partial(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, partials: torch.Tensor, *, n_seq: int,
                          seq_rows: int, n_groups: int, row0: int, group_stride: int, tok_stride: int, n_tok: int, cls_row: int, heads: int,
                          head_dim: int, scale: float, key_keep: Optional[torch.Tensor] = None):
    """`attention` + per-group partials of the CLS query into `partials` (fp32, >= n_seq*heads*n_groups*66 elements).  key_keep: optional uint8 flags per
    K/V row (0 = masked key), as in `attention`."""
    assert q.dtype == k.dtype == v.dtype == out.dtype == torch.bfloat16 and partials.dtype == torch.float32
    assert _ld(q) == _ld(k) == _ld(v) and partials.numel() >= n_seq * heads * n_groups * 66
    if key_keep is not None:
        assert key_keep.dtype == torch.uint8 and key_keep.numel() >= n_seq * seq_rows
        rc = _lib.load().sf_attention_cls_partial_masked(_dev(q, 'q'), _dev(k, 'k'), _dev(v, 'v'), _ld(q), _dev(out, 'out'), _ld(out), n_seq, seq_rows,
                                                         n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim, float(scale),
                                                         _dev(partials, 'partials'), _dev(key_keep, 'key_keep'), _stream())
        _lib.check(rc, 'sf_attention_cls_partial_masked')
        return out
    rc = _lib.load().sf_attention_cls_partial(_dev(q, 'q'), _dev(k, 'k'), _dev(v, 'v'), _ld(q), _dev(out, 'out'), _ld(out), n_seq, seq_rows,
                                              n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim, float(scale),
                                              _dev(partials, 'partials'), _stream())
    _lib.check(rc, 'sf_attention_cls_partial')
    return out


def qkv_time_attention(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], qkv_cls: torch.Tensor, out: torch.Tensor, partials: torch.Tensor, *,
                       n_seq: int, n_groups: int, scale: float, key_keep: Optional[torch.Tensor] = None):
    """Temporal qkv projection + time attention of every patch token in one launch (sf_qkv_time_attention): x (n_seq * (1 + 8 n_groups), 768) bf16,
    w (2304, 768) bf16, qkv_cls (n_seq, 2304) bf16 = the projection of the CLS rows; out: patch rows of the attention output, partials: the CLS
    query's softmax partials, one per 4 patches, for attention_cls_combine(n_part=n_groups // 4)."""
    assert x.dtype == w.dtype == qkv_cls.dtype == out.dtype == torch.bfloat16 and partials.dtype == torch.float32
    assert x.shape[1] == 768 and tuple(w.shape) == (2304, 768) and qkv_cls.shape[0] >= n_seq and qkv_cls.shape[1] == 2304 and out.shape[1] == 768
    assert x.shape[0] >= n_seq * (1 + 8 * n_groups) and out.shape[0] >= n_seq * (1 + 8 * n_groups) and partials.numel() >= n_seq * 12 * (n_groups // 4) * 66 and n_groups % 4 == 0
    if key_keep is not None:                                   # token masks: one uint8 per row of x, 0 = masked key
        assert key_keep.dtype == torch.uint8 and key_keep.numel() >= n_seq * (1 + 8 * n_groups)
        rc = _lib.load().sf_qkv_time_attention_masked(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None,
                                                      _dev(qkv_cls, 'qkv_cls'), _ld(qkv_cls), _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq,
                                                      n_groups, float(scale), _dev(key_keep, 'key_keep'), _stream())
        _lib.check(rc, 'sf_qkv_time_attention_masked')
        return out
    rc = _lib.load().sf_qkv_time_attention(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None,
                                           _dev(qkv_cls, 'qkv_cls'), _ld(qkv_cls), _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq, n_groups,
                                           float(scale), _stream())
    _lib.check(rc, 'sf_qkv_time_attention')
    return out


def copy_rows_bf16(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, src_map: RowMap = None, dst_map: RowMap = None):
    """dst[dst_map(r), :cols] = src[src_map(r), :cols] for r < rows (bf16, cols % 8 == 0; sf_copy_rows_bf16)."""
    assert src.dtype == dst.dtype == torch.bfloat16
    rc = _lib.load().sf_copy_rows_bf16(_dev(src, 'src'), _ld(src), _map(src_map), _dev(dst, 'dst'), _ld(dst), _map(dst_map), rows, cols, _stream())
    _lib.check(rc, 'sf_copy_rows_bf16')
    return dst


def space_side_rows(x: torch.Tensor, side_in: torch.Tensor, n_seq: int, seq_rows: int = 1569, n_tok: int = 196):
    """The rows qkv_space_attention / qkv_time_attention2 do NOT project themselves, gathered for one small GEMM: per sequence [the CLS row; for frame f its tokens 192 .. 195]
    -> side_in (n_seq * 33, 768) bf16 (row seq * 33, rows seq * 33 + 1 + 4 f + i).  One launch (sf_side_rows)."""
    assert x.dtype == side_in.dtype == torch.bfloat16 and x.shape[1] == side_in.shape[1] == 768 and seq_rows == 1 + 8 * n_tok
    assert x.shape[0] >= n_seq * seq_rows and side_in.shape[0] >= n_seq * 33
    rc = _lib.load().sf_side_rows(_dev(x, 'x'), _ld(x) * 2, _dev(side_in, 'side_in'), _ld(side_in) * 2, 1536, None, 0, None, 0, 0, n_seq, n_tok, _stream())
    _lib.check(rc, 'sf_side_rows')
    return side_in


def space_side_rows_mx(x_q: torch.Tensor, x_s: torch.Tensor, side_q: torch.Tensor, side_s: torch.Tensor, n_seq: int, n_tok: int = 196):
    """space_side_rows of an MXFP8 operand: the e4m3 rows x_q (rows, 768) uint8 AND their E8M0 scale dwords x_s (6, >= rows, 4) -> side_q (n_seq * 33, 768), side_s
    (6, >= n_seq * 33, 4), in the same launch."""
    assert x_q.dtype == x_s.dtype == side_q.dtype == side_s.dtype == torch.uint8 and x_q.shape[1] == side_q.shape[1] == 768
    assert x_s.dim() == 3 and side_s.dim() == 3 and x_s.shape[0] == side_s.shape[0] == 6 and x_s.is_contiguous() and side_s.is_contiguous()
    rows = n_seq * (1 + 8 * n_tok)
    assert x_q.shape[0] >= rows and x_s.shape[1] >= rows and side_q.shape[0] >= n_seq * 33 and side_s.shape[1] >= n_seq * 33
    rc = _lib.load().sf_side_rows(_dev(x_q, 'x_q'), _ld(x_q), _dev(side_q, 'side_q'), _ld(side_q), 768, _dev(x_s, 'x_s'), x_s.stride(0), _dev(side_s, 'side_s'),
                                  side_s.stride(0), 6, n_seq, n_tok, _stream())
    _lib.check(rc, 'sf_side_rows')
    return side_q, side_s


def qkv_space_attention(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], side: torch.Tensor, out: torch.Tensor, partials: torch.Tensor, *, n_seq: int,
                        scale: float, n_tok: int = 196, key_keep: Optional[torch.Tensor] = None):
    """Spatial qkv projection + space attention of every patch token in one launch (sf_qkv_space_attention): x (n_seq * 1569, 768) bf16, w (2304, 768) bf16,
    side (n_seq * 33, 2304) bf16 = the projection of the rows of space_side_rows(); out: patch rows of the attention output (a buffer of its own), partials: the CLS
    query's softmax partials, one per frame, for attention_cls_combine(n_part=8).  key_keep (uint8, one flag per row of x; 0 = masked key): the token-mask form
    (sf_qkv_space_attention_masked)."""
    assert x.dtype == w.dtype == side.dtype == out.dtype == torch.bfloat16 and partials.dtype == torch.float32
    rows = n_seq * (1 + 8 * n_tok)
    assert x.shape[1] == 768 and tuple(w.shape) == (2304, 768) and side.shape[0] >= n_seq * 33 and side.shape[1] == 2304 and out.shape[1] == 768
    assert x.shape[0] >= rows and out.shape[0] >= rows and partials.numel() >= n_seq * 12 * 8 * 66 and x.data_ptr() != out.data_ptr()
    if key_keep is not None:
        assert key_keep.dtype == torch.uint8 and key_keep.numel() >= rows and key_keep.is_contiguous()
        rc = _lib.load().sf_qkv_space_attention_masked(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'),
                                                       _ld(side), _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq, n_tok, float(scale),
                                                       _dev(key_keep, 'key_keep'), _stream())
        _lib.check(rc, 'sf_qkv_space_attention_masked')
        return out
    rc = _lib.load().sf_qkv_space_attention(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'), _ld(side),
                                            _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq, n_tok, float(scale), _stream())
    _lib.check(rc, 'sf_qkv_space_attention')
    return out


def qkv_time_attention2(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], side: torch.Tensor, out: torch.Tensor, partials: torch.Tensor, *, n_seq: int,
                        scale: float, n_tok: int = 196, key_keep: Optional[torch.Tensor] = None):
    """Temporal qkv projection + time attention of every patch token in one launch on the 192 x 384 main loop (sf_qkv_time_attention2): x (n_seq * 1569, 768) bf16,
    w (2304, 768) bf16, side (n_seq * 33, 2304) bf16 = the projection of the rows of space_side_rows(); out: patch rows of the attention output (a buffer of its own),
    partials: the CLS query's softmax partials, 33 per sequence and head, for attention_cls_combine(n_part=33)."""
    assert x.dtype == w.dtype == side.dtype == out.dtype == torch.bfloat16 and partials.dtype == torch.float32
    rows = n_seq * (1 + 8 * n_tok)
    assert x.shape[1] == 768 and tuple(w.shape) == (2304, 768) and side.shape[0] >= n_seq * 33 and side.shape[1] == 2304 and out.shape[1] == 768
    assert x.shape[0] >= rows and out.shape[0] >= rows and partials.numel() >= n_seq * 12 * 33 * 66 and x.data_ptr() != out.data_ptr()
    if key_keep is not None:                                # token masks (sf_qkv_time_attention2_masked): uint8, one flag per row of x, 0 = masked key
        assert key_keep.dtype == torch.uint8 and key_keep.numel() >= rows and key_keep.is_contiguous()
        rc = _lib.load().sf_qkv_time_attention2_masked(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'),
                                                       _ld(side), _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq, n_tok, float(scale),
                                                       _dev(key_keep, 'key_keep'), _stream())
        _lib.check(rc, 'sf_qkv_time_attention2_masked')
        return out
    rc = _lib.load().sf_qkv_time_attention2(_dev(x, 'x'), _ld(x), _dev(w, 'w'), _ld(w), _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'), _ld(side),
                                            _dev(out, 'out'), _ld(out), _dev(partials, 'partials'), n_seq, n_tok, float(scale), _stream())
    _lib.check(rc, 'sf_qkv_time_attention2')
    return out


def qkv_space_attention_mx(x_q: torch.Tensor, x_s: torch.Tensor, w_q: torch.Tensor, w_s: torch.Tensor, bias: Optional[torch.Tensor], side: torch.Tensor, out: torch.Tensor,
                           partials: torch.Tensor, *, n_seq: int, scale: float, out_scales: Optional[torch.Tensor] = None, n_tok: int = 196):
    """qkv_space_attention on MXFP8 operands: x_q (n_seq * 1569, 768) uint8 e4m3 + x_s (6, >= rows, 4) scale planes, w_q (2304, 768) + w_s (6, >= 2304, 4); side
    (n_seq * 33, 2304) bf16.  With a uint8 `out` and `out_scales` (6, >= rows, 4) the patch rows are written as MXFP8 (= quantize_mxfp8 of the bf16 output; buffers of
    their own, not x_q / x_s), else `out` is bf16."""
    assert x_q.dtype == w_q.dtype == x_s.dtype == w_s.dtype == torch.uint8 and side.dtype == torch.bfloat16 and partials.dtype == torch.float32
    assert (out.dtype == torch.uint8) == (out_scales is not None) and out.dtype in (torch.uint8, torch.bfloat16)
    rows = n_seq * (1 + 8 * n_tok)
    assert x_q.shape[1] == 768 and tuple(w_q.shape) == (2304, 768) and side.shape[0] >= n_seq * 33 and side.shape[1] == 2304 and out.shape[1] == 768
    assert x_q.shape[0] >= rows and out.shape[0] >= rows and x_s.dim() == 3 and w_s.dim() == 3 and x_s.shape[0] == 6 and w_s.shape[0] == 6
    assert x_s.shape[1] >= rows and w_s.shape[1] >= 2304 and x_s.is_contiguous() and w_s.is_contiguous() and partials.numel() >= n_seq * 12 * 8 * 66
    if out_scales is not None:
        assert out_scales.dtype == torch.uint8 and out_scales.dim() == 3 and out_scales.shape[0] == 6 and out_scales.shape[1] >= rows and out_scales.is_contiguous()
        assert out.data_ptr() != x_q.data_ptr() and out_scales.data_ptr() != x_s.data_ptr()
    rc = _lib.load().sf_qkv_space_attention_mx(_dev(x_q, 'x_q'), _ld(x_q), _dev(x_s, 'x_s'), x_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                               _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'), _ld(side),
                                               _dev(out, 'out') if out_scales is None else None, _ld(out) if out_scales is None else 0,
                                               _dev(out, 'out') if out_scales is not None else None, _ld(out) if out_scales is not None else 0,
                                               _dev(out_scales, 'out_scales') if out_scales is not None else None, out_scales.stride(0) if out_scales is not None else 0,
                                               _dev(partials, 'partials'), n_seq, n_tok, float(scale), _stream())
    _lib.check(rc, 'sf_qkv_space_attention_mx')
    return out


def qkv_time_attention2_mx(x_q: torch.Tensor, x_s: torch.Tensor, w_q: torch.Tensor, w_s: torch.Tensor, bias: Optional[torch.Tensor], side: torch.Tensor, out: torch.Tensor,
                           partials: torch.Tensor, *, n_seq: int, scale: float, out_scales: Optional[torch.Tensor] = None, n_tok: int = 196):
    """qkv_time_attention2 on MXFP8 operands (arguments as qkv_space_attention_mx; partials: 33 records per sequence and head for attention_cls_combine(_mx)(n_part=33)).
    With a uint8 `out` and `out_scales` (6, >= rows, 4) the patch rows are written as MXFP8 (= quantize_mxfp8 of the bf16 output), else `out` is bf16."""
    assert x_q.dtype == w_q.dtype == x_s.dtype == w_s.dtype == torch.uint8 and side.dtype == torch.bfloat16 and partials.dtype == torch.float32
    assert (out.dtype == torch.uint8) == (out_scales is not None) and out.dtype in (torch.uint8, torch.bfloat16)
    rows = n_seq * (1 + 8 * n_tok)
    assert x_q.shape[1] == 768 and tuple(w_q.shape) == (2304, 768) and side.shape[0] >= n_seq * 33 and side.shape[1] == 2304 and out.shape[1] == 768
    assert x_q.shape[0] >= rows and out.shape[0] >= rows and x_s.dim() == 3 and w_s.dim() == 3 and x_s.shape[0] == 6 and w_s.shape[0] == 6
    assert x_s.shape[1] >= rows and w_s.shape[1] >= 2304 and x_s.is_contiguous() and w_s.is_contiguous() and partials.numel() >= n_seq * 12 * 33 * 66
    if out_scales is not None:
        assert out_scales.dtype == torch.uint8 and out_scales.dim() == 3 and out_scales.shape[0] == 6 and out_scales.shape[1] >= rows and out_scales.is_contiguous()
        assert out.data_ptr() != x_q.data_ptr() and out_scales.data_ptr() != x_s.data_ptr()
    rc = _lib.load().sf_qkv_time_attention2_mx(_dev(x_q, 'x_q'), _ld(x_q), _dev(x_s, 'x_s'), x_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                               _dev(bias, 'bias') if bias is not None else None, _dev(side, 'side'), _ld(side),
                                               _dev(out, 'out') if out_scales is None else None, _ld(out) if out_scales is None else 0,
                                               _dev(out, 'out') if out_scales is not None else None, _ld(out) if out_scales is not None else 0,
                                               _dev(out_scales, 'out_scales') if out_scales is not None else None, out_scales.stride(0) if out_scales is not None else 0,
                                               _dev(partials, 'partials'), n_seq, n_tok, float(scale), _stream())
    _lib.check(rc, 'sf_qkv_time_attention2_mx')
    return out


def qkv_time_attention_mx(x_q: torch.Tensor, x_s: torch.Tensor, w_q: torch.Tensor, w_s: torch.Tensor, bias: Optional[torch.Tensor], qkv_cls: torch.Tensor,
                          out: torch.Tensor, partials: torch.Tensor, *, n_seq: int, n_groups: int, scale: float, out_scales: Optional[torch.Tensor] = None):
    """qkv_time_attention on MXFP8 operands: x_q (n_seq * (1 + 8 n_groups), 768) uint8 e4m3 + x_s (6, >= rows, 4) scale planes, w_q (2304, 768) + w_s (6, >= 2304, 4);
    qkv_cls (n_seq, 2304) bf16, out bf16, partials fp32 as in qkv_time_attention.  With a uint8 `out` and `out_scales` (6, >= rows, 4) the patch rows are written
    as MXFP8 (= quantize_mxfp8 of the bf16 output; buffers of their own, not x_q / x_s)."""
    assert x_q.dtype == w_q.dtype == x_s.dtype == w_s.dtype == torch.uint8 and qkv_cls.dtype == torch.bfloat16 and partials.dtype == torch.float32
    assert (out.dtype == torch.uint8) == (out_scales is not None) and out.dtype in (torch.uint8, torch.bfloat16)
    assert x_q.shape[1] == 768 and tuple(w_q.shape) == (2304, 768) and qkv_cls.shape[0] >= n_seq and qkv_cls.shape[1] == 2304 and out.shape[1] == 768
    rows = n_seq * (1 + 8 * n_groups)
    assert x_q.shape[0] >= rows and out.shape[0] >= rows and x_s.dim() == 3 and w_s.dim() == 3 and x_s.shape[0] == 6 and w_s.shape[0] == 6
    assert x_s.shape[1] >= rows and w_s.shape[1] >= 2304 and x_s.is_contiguous() and w_s.is_contiguous() and partials.numel() >= n_seq * 12 * (n_groups // 4) * 66
    if out_scales is not None:
        assert out_scales.dtype == torch.uint8 and out_scales.dim() == 3 and out_scales.shape[0] == 6 and out_scales.shape[1] >= rows and out_scales.is_contiguous()
        assert out.data_ptr() != x_q.data_ptr() and out_scales.data_ptr() != x_s.data_ptr()
        rc = _lib.load().sf_qkv_time_attention_mx_q(_dev(x_q, 'x_q'), _ld(x_q), _dev(x_s, 'x_s'), x_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                                    _dev(bias, 'bias') if bias is not None else None, _dev(qkv_cls, 'qkv_cls'), _ld(qkv_cls), _dev(out, 'out'), _ld(out),
                                                    _dev(out_scales, 'out_scales'), out_scales.stride(0), _dev(partials, 'partials'), n_seq, n_groups, float(scale), _stream())
        _lib.check(rc, 'sf_qkv_time_attention_mx_q')
        return out
    rc = _lib.load().sf_qkv_time_attention_mx(_dev(x_q, 'x_q'), _ld(x_q), _dev(x_s, 'x_s'), x_s.stride(0), _dev(w_q, 'w_q'), _ld(w_q), _dev(w_s, 'w_s'), w_s.stride(0),
                                              _dev(bias, 'bias') if bias is not None else None, _dev(qkv_cls, 'qkv_cls'), _ld(qkv_cls), _dev(out, 'out'), _ld(out),
                                              _dev(partials, 'partials'), n_seq, n_groups, float(scale), _stream())
    _lib.check(rc, 'sf_qkv_time_attention_mx')
    return out


def attention_cls_partial_mx(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out_q: torch.Tensor, out_s: torch.Tensor, partials: torch.Tensor, *, n_seq: int,
                             seq_rows: int, n_groups: int, row0: int, group_stride: int, tok_stride: int, n_tok: int, cls_row: int, heads: int, scale: float):
    """`attention_cls_partial` (head_dim 64, 193 <= n_tok <= 207) writing MXFP8: out_q uint8 (rows, heads*64), out_s uint8 scale planes (heads*64/128, rows_padded, 4)
    as `mx_scale_planes` lays them out - byte for byte what `quantize_mxfp8` makes of the bf16 output."""
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and out_q.dtype == out_s.dtype == torch.uint8 and partials.dtype == torch.float32
    assert _ld(q) == _ld(k) == _ld(v) and partials.numel() >= n_seq * heads * n_groups * 66 and out_s.dim() == 3 and out_s.shape[0] * 2 == heads
    rc = _lib.load().sf_attention_cls_partial_mx(_dev(q, 'q'), _dev(k, 'k'), _dev(v, 'v'), _ld(q), _dev(out_q, 'out_q'), _ld(out_q), _dev(out_s, 'out_s'), out_s.stride(0),
                                                 n_seq, seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, float(scale),
                                                 _dev(partials, 'partials'), _stream())
    _lib.check(rc, 'sf_attention_cls_partial_mx')
    return out_q


def attention_cls_combine_mx(partials: torch.Tensor, out_q: torch.Tensor, out_s: torch.Tensor, *, n_part: int, n_seq: int, out_seq_rows: int, out_row: int, heads: int):
    """`attention_cls_combine` writing the CLS rows as MXFP8 into the buffers of `attention_cls_partial_mx`."""
    assert out_q.dtype == out_s.dtype == torch.uint8 and out_s.dim() == 3 and out_s.shape[0] * 2 == heads
    rc = _lib.load().sf_attention_cls_combine_mx(_dev(partials, 'partials'), n_part, _dev(out_q, 'out_q'), _ld(out_q), _dev(out_s, 'out_s'), out_s.stride(0), out_seq_rows,
                                                 out_row, n_seq, heads, _stream())
    _lib.check(rc, 'sf_attention_cls_combine_mx')
    return out_q


def attention_cls_combine(partials: torch.Tensor, out: torch.Tensor, *, n_part: int, n_seq: int, out_seq_rows: int, out_row: int, heads: int):
    rc = _lib.load().sf_attention_cls_combine(_dev(partials, 'partials'), n_part, _dev(out, 'out'), _ld(out), out_seq_rows, out_row, n_seq, heads,
                                              _stream())
    _lib.check(rc, 'sf_attention_cls_combine')
    return out


def attention_cls(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, n_seq: int, q_seq_rows: int,
                  q_row: int, kv_seq_rows: int, kv_row0: int, n_keys: int, out_seq_rows: int, out_row: int, heads: int,
                  head_dim: int, scale: float, key_keep: Optional[torch.Tensor] = None):
    assert q.dtype == k.dtype == v.dtype == out.dtype == torch.bfloat16
    assert _ld(q) == _ld(k) == _ld(v)
    if key_keep is None:
        rc = _lib.load().sf_attention_cls(_dev(q, 'q'), q_seq_rows, q_row, _dev(k, 'k'), _dev(v, 'v'), _ld(q), kv_seq_rows,
                                          kv_row0, n_keys, _dev(out, 'out'), _ld(out), out_seq_rows, out_row, n_seq, heads,
                                          head_dim, float(scale), _stream())
    else:
        assert key_keep.dtype == torch.uint8 and key_keep.is_contiguous()
        rc = _lib.load().sf_attention_cls_masked(_dev(q, 'q'), q_seq_rows, q_row, _dev(k, 'k'), _dev(v, 'v'), _ld(q), kv_seq_rows,
                                                 kv_row0, n_keys, _dev(out, 'out'), _ld(out), out_seq_rows, out_row, n_seq, heads,
                                                 head_dim, float(scale), _dev(key_keep, 'key_keep'), _stream())
    _lib.check(rc, 'sf_attention_cls')
    return out


def agg_cls_pool(x: torch.Tensor, out: torch.Tensor, *, n_seq: int, seq_rows: int, row0: int, n_groups: int, group_stride: int, tok_stride: int, n_tok: int,
                 norm_a, eps_a: float, norm_b, eps_b: float, u: torch.Tensor, c: torch.Tensor, zn_cls: torch.Tensor, key_keep: Optional[torch.Tensor] = None):
    """The aggregator's CLS-query attention pooled in one pass over x (sf_agg_cls_pool): out bf16 (n_seq, 12 * 2 * 768), out[sq, h] = (hi | lo) of sum_j softmax_j(u[h] . zn_j + c[h]) zn_j
    (hi = bf16 of the fp32 sum, lo = bf16 of the rest; a GEMM against [W | W] sees the sum at ~16 bits) over the keys [zn_cls; zn of the sequence's n_tok token rows], zn = bf16(LN_b(LN_a(x row))).  norm_a / norm_b: (gamma, beta) fp32 pairs; u (12, 768), c (12,),
    zn_cls (768,) fp32; key_keep uint8, one flag per row of x.  n_seq counts pooled sequences (segments * n_groups)."""
    assert x.dtype == torch.float32 and x.shape[1] == 768 and out.dtype == torch.bfloat16 and out.shape[1] == 12 * 2 * 768 and out.shape[0] >= n_seq
    assert n_seq % n_groups == 0 and row0 + (n_groups - 1) * group_stride + max(n_tok - 1, 0) * tok_stride < seq_rows and x.shape[0] >= (n_seq // n_groups) * seq_rows
    for t, n in ((norm_a[0], 768), (norm_a[1], 768), (norm_b[0], 768), (norm_b[1], 768), (u, 12 * 768), (c, 12), (zn_cls, 768)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    if key_keep is not None:
        assert key_keep.dtype == torch.uint8 and key_keep.is_contiguous() and key_keep.numel() >= (n_seq // n_groups) * seq_rows
    rc = _lib.load().sf_agg_cls_pool(_dev(x, 'x'), _ld(x), n_seq, seq_rows, row0, n_groups, group_stride, tok_stride, n_tok,
                                     _dev(norm_a[0], 'gamma1'), _dev(norm_a[1], 'beta1'), float(eps_a), _dev(norm_b[0], 'gamma2'), _dev(norm_b[1], 'beta2'), float(eps_b),
                                     _dev(u, 'u'), _dev(c, 'c'), _dev(zn_cls, 'zn_cls'), _dev(key_keep, 'key_keep') if key_keep is not None else None,
                                     _dev(out, 'out'), _ld(out), _stream())
    _lib.check(rc, 'sf_agg_cls_pool')
    return out


def token_mask_video(content_keep: torch.Tensor, w0_sign: torch.Tensor, out: torch.Tensor):
    """content_keep (n, 16, 3, 224, 224) bool|uint8 (True = kept) -> out uint8 (n*1569,) token keep flags (CLS kept)."""
    m = content_keep.contiguous().view(torch.uint8)
    rc = _lib.load().sf_token_mask_video(_dev(m, 'mask'), m.shape[0], _dev(w0_sign, 'w0_sign'), _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_token_mask_video')
    return out


def token_mask_spec(content_keep: torch.Tensor, w0_sign: torch.Tensor, out: torch.Tensor):
    """content_keep (n, F, Ta) bool|uint8 -> out uint8 (n*74,) token keep flags (CLS, DISTILL kept)."""
    m = content_keep.contiguous().view(torch.uint8)
    rc = _lib.load().sf_token_mask_spec(_dev(m, 'mask'), m.shape[0], m.shape[1], m.shape[2], _dev(w0_sign, 'w0_sign'), _dev(out, 'out'), _stream())
    _lib.check(rc, 'sf_token_mask_spec')
    return out


def meanpool_l2norm(x: torch.Tensor, out: torch.Tensor, t: int, normalize: bool):
    """x (n*t, 768) fp32 -> out (n, 768): mean over each run of t rows, then optional F.normalize (open_clip/model.py:530-531)."""
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.shape[0] == out.shape[0] * t
    rc = _lib.load().sf_meanpool_l2norm768(_dev(x, 'x'), _ld(x), t, _dev(out, 'out'), _ld(out), int(bool(normalize)), out.shape[0], _stream())
    _lib.check(rc, 'sf_meanpool_l2norm768')
    return out


def similarity(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, scale: float):
    """out (n, m) = scale * a (n, d) @ b (m, d)^T in fp32 (open_clip/model.py:508-509)."""
    assert a.dtype == b.dtype == out.dtype == torch.float32 and a.shape[1] == b.shape[1]
    rc = _lib.load().sf_similarity_f32(_dev(a, 'a'), _ld(a), _dev(b, 'b'), _ld(b), _dev(out, 'out'), _ld(out), a.shape[0], b.shape[0],
                                       a.shape[1], float(scale), _stream())
    _lib.check(rc, 'sf_similarity_f32')
    return out


def cross_entropy(logits: torch.Tensor, targets: torch.Tensor, loss: torch.Tensor, dlogits: torch.Tensor = None):
    """loss[0] = F.cross_entropy(logits, targets) (mean) for fp32 (B, C) logits and int64 class targets; optionally
    dlogits = d loss / d logits in the same launch.  A target outside [0, C) gives a NaN loss (and a zero dlogits row)."""
    assert logits.dtype == torch.float32 and targets.dtype == torch.int64 and loss.dtype == torch.float32
    assert dlogits is None or (dlogits.dtype == torch.float32 and dlogits.shape == logits.shape)
    rc = _lib.load().sf_cross_entropy(_dev(logits, 'logits'), _ld(logits), _dev(targets, 'targets'), logits.shape[0], logits.shape[1],
                                      _dev(loss, 'loss'), _dev(dlogits, 'dlogits') if dlogits is not None else None,
                                      _ld(dlogits) if dlogits is not None else 0, 1.0, _stream())
    _lib.check(rc, 'sf_cross_entropy')
    return loss


def track_decode(logits: torch.Tensor, lam: float):
    """Track read-out of a recording's window logits (sf_track_decode): logits fp32 (W, C) on device, rows in time order, 2 <= C <= 64 ->
    (cls_raw int32 (W,), conf_raw fp32 (W,), cls_path int32 (W,), conf_path fp32 (W,)): the per-window argmax and its softmax probability, and the
    Viterbi path under a cost `lam` per class step with the softmax probability of the path's class.  Allocates the W * C bytes of back pointers."""
    assert logits.dtype == torch.float32 and logits.dim() == 2
    W, C = logits.shape
    dev = logits.device
    cls_raw, cls_path = torch.empty(W, device=dev, dtype=torch.int32), torch.empty(W, device=dev, dtype=torch.int32)
    conf_raw, conf_path = torch.empty(W, device=dev, dtype=torch.float32), torch.empty(W, device=dev, dtype=torch.float32)
    back = torch.empty(max(W, 1) * C, device=dev, dtype=torch.uint8)
    rc = _lib.load().sf_track_decode(_dev(logits, 'logits'), _ld(logits) if W else C, W, C, float(lam), _dev(cls_raw, 'cls_raw'), _dev(conf_raw, 'conf_raw'),
                                     _dev(cls_path, 'cls_path'), _dev(conf_path, 'conf_path'), _dev(back, 'backptr'), _stream())
    _lib.check(rc, 'sf_track_decode')
    return cls_raw, conf_raw, cls_path, conf_path


def track_posterior(logits: torch.Tensor, lam: float, grid: torch.Tensor, post: Optional[torch.Tensor] = None):
    """Posterior (forward-backward) read-out of a recording's window logits (sf_track_posterior): logits fp32 (W, C) on device with unit column stride (a row
    stride above C is passed on), rows in time order, 2 <= C <= 64; grid fp32 (C,) on the same device: the offsets the classes stand for ->
    (post fp32 (W, C), cls_post int32 (W,), conf_post fp32 (W,), offset_mean fp32 (W,), log_z fp32 (1,)): the marginals of the chain whose mode is
    track_decode's path, their argmax and its value, the posterior mean of the grid, and the log partition sum over independent softmax draws (<= 0).
    Allocates the outputs and the 2 W C floats of workspace (`post`, if given, is written instead of a fresh tensor: fp32 (W, C) with unit column stride, any
    row stride >= C); nothing is read back: log_z stays on the device (0 for W = 0, the empty product)."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and grid.dtype == torch.float32 and grid.device == logits.device
    W, C = logits.shape
    assert grid.dim() == 1 and grid.numel() == C and grid.is_contiguous(), f'a grid of {tuple(grid.shape)} for {C} classes'
    assert W == 0 or logits.stride(1) == 1, 'logits: unit column stride'
    dev = logits.device
    if post is None:
        post = torch.empty(W, C, device=dev, dtype=torch.float32)
    assert post.dtype == torch.float32 and post.shape == (W, C) and post.device == dev and (W == 0 or post.stride(1) == 1), 'post: fp32 (W, C), unit column stride'
    cls_post = torch.empty(W, device=dev, dtype=torch.int32)
    conf_post, offset_mean = torch.empty(W, device=dev, dtype=torch.float32), torch.empty(W, device=dev, dtype=torch.float32)
    log_z = torch.empty(1, device=dev, dtype=torch.float32) if W else torch.zeros(1, device=dev, dtype=torch.float32)
    ws = torch.empty(2 * max(W, 1) * C, device=dev, dtype=torch.float32)
    rc = _lib.load().sf_track_posterior(_dev(logits, 'logits'), _ld(logits) if W else C, W, C, float(lam), _dev(grid, 'grid'), _dev(post, 'post'), _ld(post) if W else C,
                                        _dev(cls_post, 'cls_post'), _dev(conf_post, 'conf_post'), _dev(offset_mean, 'offset_mean'), _dev(log_z, 'log_z'),
                                        _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_posterior')
    return post, cls_post, conf_post, offset_mean, log_z


def _gated_inputs(logits: torch.Tensor, gate_logits: torch.Tensor):
    """The shape checks the two gated read-outs share -> (W, C): logits fp32 (W, C), gate_logits fp32 (W, 2), same device, unit column stride, any row stride."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and gate_logits.dtype == torch.float32 and gate_logits.device == logits.device
    W, C = logits.shape
    assert gate_logits.shape == (W, 2), f'gate logits of {tuple(gate_logits.shape)} for {W} windows'
    assert W == 0 or (logits.stride(1) == 1 and gate_logits.stride(1) == 1), 'logits, gate_logits: unit column stride'
    return W, C


def track_decode_gated(logits: torch.Tensor, gate_logits: torch.Tensor, lam: float, mu: float):
    """Track read-out gated by synchronizability (sf_track_decode_gated): logits fp32 (W, C) of the offset head and gate_logits fp32 (W, 2) of the 2-way
    syncability head (class 1 = synchronizable) for the same windows, on one device, rows in time order, unit column stride (a row stride above the width is passed
    on), 2 <= C <= 32 -> (cls_raw int32, conf_raw fp32, sync_raw fp32, cls_path int32, sync_path int32, conf_path fp32), (W,) each: the per-window argmax and its
    softmax probability as track_decode gives them, sigmoid(z1 - z0), and the Viterbi path of the chain over (offset class, synchronizable flag) under a cost `lam`
    per class step and `mu` per change of the flag, with the softmax probability of the path's class.  Allocates the outputs and the W * 2C bytes of back pointers."""
    W, C = _gated_inputs(logits, gate_logits)
    dev = logits.device
    i32 = lambda: torch.empty(W, device=dev, dtype=torch.int32)
    f32 = lambda: torch.empty(W, device=dev, dtype=torch.float32)
    cls_raw, cls_path, sync_path = i32(), i32(), i32()
    conf_raw, sync_raw, conf_path = f32(), f32(), f32()
    back = torch.empty(max(W, 1) * 2 * C, device=dev, dtype=torch.uint8)
    rc = _lib.load().sf_track_decode_gated(_dev(logits, 'logits'), _ld(logits) if W else C, _dev(gate_logits, 'gate_logits'), _ld(gate_logits) if W else 2, W, C,
                                           float(lam), float(mu), _dev(cls_raw, 'cls_raw'), _dev(conf_raw, 'conf_raw'), _dev(sync_raw, 'sync_raw'),
                                           _dev(cls_path, 'cls_path'), _dev(sync_path, 'sync_path'), _dev(conf_path, 'conf_path'), _dev(back, 'backptr'), _stream())
    _lib.check(rc, 'sf_track_decode_gated')
    return cls_raw, conf_raw, sync_raw, cls_path, sync_path, conf_path


def track_posterior_gated(logits: torch.Tensor, gate_logits: torch.Tensor, lam: float, mu: float, grid: torch.Tensor, post: Optional[torch.Tensor] = None):
    """Posterior read-out gated by synchronizability (sf_track_posterior_gated): inputs as track_decode_gated, grid fp32 (C,) on the same device ->
    (post fp32 (W, C), p_sync fp32 (W,), cls_post int32 (W,), conf_post fp32 (W,), offset_mean fp32 (W,), log_z fp32 (1,)): the marginals of the offset class under
    the chain over (offset class, synchronizable flag), the marginal of the flag, and cls_post / conf_post / offset_mean / log_z from `post` as track_posterior
    defines them.  Allocates the outputs and the 4 W C floats of workspace (`post`, if given, is written instead of a fresh tensor: fp32 (W, C) with unit column
    stride, any row stride >= C); nothing is read back: log_z stays on the device (0 for W = 0)."""
    W, C = _gated_inputs(logits, gate_logits)
    assert grid.dtype == torch.float32 and grid.device == logits.device
    assert grid.dim() == 1 and grid.numel() == C and grid.is_contiguous(), f'a grid of {tuple(grid.shape)} for {C} classes'
    dev = logits.device
    if post is None:
        post = torch.empty(W, C, device=dev, dtype=torch.float32)
    assert post.dtype == torch.float32 and post.shape == (W, C) and post.device == dev and (W == 0 or post.stride(1) == 1), 'post: fp32 (W, C), unit column stride'
    cls_post = torch.empty(W, device=dev, dtype=torch.int32)
    p_sync, conf_post, offset_mean = (torch.empty(W, device=dev, dtype=torch.float32) for _ in range(3))
    log_z = torch.empty(1, device=dev, dtype=torch.float32) if W else torch.zeros(1, device=dev, dtype=torch.float32)
    ws = torch.empty(4 * max(W, 1) * C, device=dev, dtype=torch.float32)
    rc = _lib.load().sf_track_posterior_gated(_dev(logits, 'logits'), _ld(logits) if W else C, _dev(gate_logits, 'gate_logits'), _ld(gate_logits) if W else 2, W, C,
                                              float(lam), float(mu), _dev(grid, 'grid'), _dev(post, 'post'), _ld(post) if W else C, _dev(p_sync, 'p_sync'),
                                              _dev(cls_post, 'cls_post'), _dev(conf_post, 'conf_post'), _dev(offset_mean, 'offset_mean'), _dev(log_z, 'log_z'),
                                              _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_posterior_gated')
    return post, p_sync, cls_post, conf_post, offset_mean, log_z


TRACK_WIDE_MAX_S, TRACK_WIDE_MAX_D = 1024, 1024      # sf_track_wide.hip: one thread per state in one workgroup; lags per window


def track_wide_states(lags, grid, seg_sec: float = 0.32):
    """The states of a search over audio lags, on the host in float64: lags ascending integers (segments of seg_sec seconds), grid (C,) the offsets
    of the classes -> (state_src int32, pos fp32, off fp32, lag_of int32, cls_of int32), CPU tensors of S = D C entries.  State (lag index d, class c) stands for the
    offset seg_sec * lags[d] + grid[c] (a_start = v_start + offset_sec); offsets are taken to the microsecond, so that 0.32 * 5 - 1.6 and 0.0 coincide (precondition: grid and seg_sec in whole microseconds up to fp32
    resolution; ValueError otherwise, nothing is quantised silently).  The states
    are sorted by (offset, d, c); state_src = d * C + c, lag_of = d (the INDEX into lags), cls_of = c, off the offset in seconds, pos = off / (grid[1] - grid[0]):
    the position in class steps, which is what `lam` is charged on.  lags = (0,) with the default grid gives pos = c - 10 exactly."""
    lags = [int(d) for d in lags]
    g = torch.as_tensor(grid).detach().cpu().double()
    if len(lags) < 1 or any(b <= a for a, b in zip(lags, lags[1:])) or g.dim() != 1 or g.numel() < 2:
        raise ValueError(f'track_wide_states: lags {lags} (at least one, strictly ascending), a grid of {tuple(g.shape)}')
    C = g.numel()
    sec = [[seg_sec * d + float(g[c]) for c in range(C)] for d in lags]
    us = [[int(round(v * 1e6)) for v in row] for row in sec]
    step = int(round(float(g[1] - g[0]) * 1e6))
    if step <= 0:
        raise ValueError(f'track_wide_states: the grid steps by {float(g[1] - g[0])} s')
    # PRECONDITION: the offsets lie on the microsecond lattice up to what an fp32 grid can say (2^-22 relative, 0.24 us at 1 s).  A grid that does not - a step of
    # 1/3 s - would be quantised silently, and two of its offsets could be merged or split by the rounding: refuse it.
    worst = max(abs(u / 1e6 - v) / max(1.0, abs(v)) for ru, rv in zip(us, sec) for u, v in zip(ru, rv))
    if worst > 2.0 ** -22 or abs(step / 1e6 - float(g[1] - g[0])) > 2.0 ** -22:
        raise ValueError(f'track_wide_states: the offsets seg_sec * lag + grid[c] are taken to the microsecond, and this grid / seg_sec = {seg_sec} is off that lattice '
                         f'by up to {worst:.2e} (relative): give a grid in whole microseconds')
    order = sorted((us[j][c], j, c) for j in range(len(lags)) for c in range(C))
    key = torch.tensor([o[0] for o in order], dtype=torch.float64)
    lag_of = torch.tensor([o[1] for o in order], dtype=torch.int32)
    cls_of = torch.tensor([o[2] for o in order], dtype=torch.int32)
    return lag_of * C + cls_of, (key / step).float(), (key / 1e6).float(), lag_of, cls_of


class TrackWideTables:
    """The two tables of the wide read-outs as the launchers take them - host copies they validate, device copies the kernels read - plus the states' offsets on
    the device.  Made once (track_wide_tables), before any graph capture; the ops only pass pointers."""

    def __init__(self, state_src: torch.Tensor, pos: torch.Tensor, off: torch.Tensor, D: int, C: int, device):
        self.D, self.C, self.S = int(D), int(C), int(state_src.numel())
        self.src_host = state_src.detach().cpu().to(torch.int32).contiguous()
        self.pos_host = pos.detach().cpu().to(torch.float32).contiguous()
        off_host = off.detach().cpu().to(torch.float32).contiguous()
        if not (self.src_host.dim() == 1 and self.pos_host.shape == self.src_host.shape == off_host.shape):
            raise ValueError(f'track_wide_tables: state_src {tuple(state_src.shape)}, pos {tuple(pos.shape)}, off {tuple(off.shape)}')
        if not (2 <= self.S <= TRACK_WIDE_MAX_S and 1 <= self.D <= TRACK_WIDE_MAX_D and self.S <= self.D * self.C):
            raise ValueError(f'track_wide_tables: S = {self.S} states (2 .. {TRACK_WIDE_MAX_S}) for D = {self.D} lags (1 .. {TRACK_WIDE_MAX_D}) x C = {self.C} classes')
        self.src, self.pos, self.off = self.src_host.to(device), self.pos_host.to(device), off_host.to(device)


def track_wide_tables(state_src: torch.Tensor, pos: torch.Tensor, off: torch.Tensor, D: int, C: int, device) -> TrackWideTables:
    """state_src, pos, off as track_wide_states returns them (or any tables of the contract: S <= 1024 states in the caller's order, pos ascending) for logits
    (W, D, C) -> the tables object track_decode_wide / track_posterior_wide take.  Copies to the device (synchronous, pageable memory): not under graph capture."""
    return TrackWideTables(state_src, pos, off, D, C, device)


def _wide_inputs(who: str, logits: torch.Tensor, tables: TrackWideTables, gate_logits: Optional[torch.Tensor]):
    """The checks the two wide read-outs share -> (W, the six stride arguments): logits fp32 (W, D, C) with unit class stride, gate_logits fp32 (W, D, 2) or None."""
    assert logits.dtype == torch.float32 and logits.dim() == 3 and tuple(logits.shape[1:]) == (tables.D, tables.C), \
        f'{who}: logits {tuple(logits.shape)} for tables of D = {tables.D} lags x C = {tables.C} classes'
    assert logits.device == tables.src.device, f'{who}: logits on {logits.device}, the tables on {tables.src.device}'
    W = logits.shape[0]
    assert W == 0 or logits.stride(2) == 1, f'{who}: logits: unit class stride'
    ld = (logits.stride(0), logits.stride(1)) if W else (tables.D * tables.C, tables.C)
    lg = (2 * tables.D, 2)
    if gate_logits is not None:
        assert gate_logits.dtype == torch.float32 and gate_logits.shape == (W, tables.D, 2) and gate_logits.device == logits.device, \
            f'{who}: gate logits of {tuple(gate_logits.shape)} for {W} windows x {tables.D} lags'
        assert W == 0 or gate_logits.stride(2) == 1, f'{who}: gate_logits: unit class stride'
        if W:
            lg = (gate_logits.stride(0), gate_logits.stride(1))
    return W, ld, lg


def _wide_workspace(W: int, tables: TrackWideTables, posterior: bool, dev) -> torch.Tensor:
    n = C.c_int64(0)
    _lib.check(_lib.load().sf_track_wide_workspace_bytes(W, tables.D, tables.S, int(posterior), C.addressof(n)), 'sf_track_wide_workspace_bytes')
    return torch.empty(n.value, device=dev, dtype=torch.uint8)


def track_decode_wide(logits: torch.Tensor, tables: TrackWideTables, lam: float, gate_logits: Optional[torch.Tensor] = None):
    """The Viterbi read-out of the wide chain (sf_track_decode_wide): logits fp32 (W, D, C) on the tables' device (engine.sync_windows_lagged), rows in
    time order, unit class stride, any row and lag stride; gate_logits fp32 (W, D, 2) or None -> (state_raw int32, conf_raw fp32, state_path int32, conf_path fp32),
    (W,) each: the per-window argmax over the S states (lowest state on ties) with its softmax probability over all states, and the path under a cost `lam` per class
    step of |pos| with that probability at the path's state.  tables.lag_of / cls_of of track_wide_states map a state back.  Allocates the outputs and the workspace."""
    W, ld, lg = _wide_inputs('track_decode_wide', logits, tables, gate_logits)
    dev = logits.device
    state_raw, state_path = torch.empty(W, device=dev, dtype=torch.int32), torch.empty(W, device=dev, dtype=torch.int32)
    conf_raw, conf_path = torch.empty(W, device=dev, dtype=torch.float32), torch.empty(W, device=dev, dtype=torch.float32)
    ws = _wide_workspace(W, tables, False, dev)
    rc = _lib.load().sf_track_decode_wide(_dev(logits, 'logits'), ld[0], ld[1], None if gate_logits is None else _dev(gate_logits, 'gate_logits'), lg[0], lg[1], W,
                                          tables.D, tables.C, tables.S, tables.src_host.data_ptr(), tables.pos_host.data_ptr(), _dev(tables.src, 'state_src'),
                                          _dev(tables.pos, 'pos'), float(lam), _dev(state_raw, 'state_raw'), _dev(conf_raw, 'conf_raw'),
                                          _dev(state_path, 'state_path'), _dev(conf_path, 'conf_path'), _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_decode_wide')
    return state_raw, conf_raw, state_path, conf_path


def track_posterior_wide(logits: torch.Tensor, tables: TrackWideTables, lam: float, gate_logits: Optional[torch.Tensor] = None, post: Optional[torch.Tensor] = None):
    """The posterior read-out of the wide chain (sf_track_posterior_wide): inputs as track_decode_wide -> (post fp32 (W, S), state_post int32 (W,), conf_post fp32
    (W,), offset_mean fp32 (W,), p_lag fp32 (W, D), log_z fp32 (1,)): the marginals of the states, their argmax and its value, the posterior mean of tables.off
    (seconds), the marginal of each lag, and the log partition sum (<= W log D without a gate, with equality at lam = 0).  Allocates the outputs and the workspace (`post`, if given, is written
    instead: fp32 (W, S), unit column stride, any row stride >= S); nothing is read back: log_z stays on the device (0 for W = 0)."""
    W, ld, lg = _wide_inputs('track_posterior_wide', logits, tables, gate_logits)
    dev, S = logits.device, tables.S
    if post is None:
        post = torch.empty(W, S, device=dev, dtype=torch.float32)
    assert post.dtype == torch.float32 and post.shape == (W, S) and post.device == dev and (W == 0 or post.stride(1) == 1), 'post: fp32 (W, S), unit column stride'
    state_post = torch.empty(W, device=dev, dtype=torch.int32)
    conf_post, offset_mean = torch.empty(W, device=dev, dtype=torch.float32), torch.empty(W, device=dev, dtype=torch.float32)
    p_lag = torch.empty(W, tables.D, device=dev, dtype=torch.float32)
    log_z = torch.empty(1, device=dev, dtype=torch.float32) if W else torch.zeros(1, device=dev, dtype=torch.float32)
    ws = _wide_workspace(W, tables, True, dev)
    rc = _lib.load().sf_track_posterior_wide(_dev(logits, 'logits'), ld[0], ld[1], None if gate_logits is None else _dev(gate_logits, 'gate_logits'), lg[0], lg[1], W,
                                             tables.D, tables.C, S, tables.src_host.data_ptr(), tables.pos_host.data_ptr(), _dev(tables.src, 'state_src'),
                                             _dev(tables.pos, 'pos'), float(lam), _dev(tables.off, 'off'), _dev(post, 'post'), post.stride(0) if W else S,
                                             _dev(state_post, 'state_post'), _dev(conf_post, 'conf_post'), _dev(offset_mean, 'offset_mean'), _dev(p_lag, 'p_lag'),
                                             _dev(log_z, 'log_z'), _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_posterior_wide')
    return post, state_post, conf_post, offset_mean, p_lag, log_z


def _pairwise_outputs(W: int, C: int, dev, xi: bool, n_float: int):
    """The outputs the two pairwise read-outs share: n_float fp32 vectors and top_from / top_to int32 of W - 1 rows, xi (W - 1, C, C) or None, log_z (1,)."""
    n = max(W - 1, 0)
    floats = [torch.empty(n, device=dev, dtype=torch.float32) for _ in range(n_float)]
    top_from, top_to = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
    xi_t = torch.empty(n, C, C, device=dev, dtype=torch.float32) if xi else None
    log_z = torch.empty(1, device=dev, dtype=torch.float32) if W else torch.zeros(1, device=dev, dtype=torch.float32)
    return floats, top_from, top_to, xi_t, log_z


def track_pairwise(logits: torch.Tensor, lam: float, xi: bool = False):
    """Pairwise marginals of neighbouring windows (sf_track_pairwise): logits as track_posterior takes them ->
    (p_change fp32 (W-1,), jump_abs fp32 (W-1,), top_from int32 (W-1,), top_to int32 (W-1,), p_top fp32 (W-1,), xi fp32 (W-1, C, C) or None, log_z fp32 (1,)):
    per boundary between windows w and w + 1, given all windows, the probability that the class changes, the expected class step |c_{w+1} - c_w|, the likeliest
    change (from class, to class) with its probability, and with xi=True the whole joint marginal xi[w, p, c] = P(c_w = p, c_{w+1} = c).  log_z is
    track_posterior's, bit for bit.  Allocates the outputs and the 2 W C floats of workspace; nothing is read back (log_z is 0 for W = 0)."""
    assert logits.dtype == torch.float32 and logits.dim() == 2
    W, C = logits.shape
    assert W == 0 or logits.stride(1) == 1, 'logits: unit column stride'
    dev = logits.device
    (p_change, jump_abs, p_top), top_from, top_to, xi_t, log_z = _pairwise_outputs(W, C, dev, xi, 3)
    ws = torch.empty(2 * max(W, 1) * C, device=dev, dtype=torch.float32)
    rc = _lib.load().sf_track_pairwise(_dev(logits, 'logits'), _ld(logits) if W else C, W, C, float(lam), _dev(p_change, 'p_change'), _dev(jump_abs, 'jump_abs'),
                                       _dev(top_from, 'top_from'), _dev(top_to, 'top_to'), _dev(p_top, 'p_top'), _dev(xi_t, 'xi') if xi else None,
                                       _dev(log_z, 'log_z'), _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_pairwise')
    return p_change, jump_abs, top_from, top_to, p_top, xi_t, log_z


def track_pairwise_gated(logits: torch.Tensor, gate_logits: torch.Tensor, lam: float, mu: float, xi: bool = False):
    """Pairwise marginals under the chain over (offset class, synchronizable flag) (sf_track_pairwise_gated): inputs as track_decode_gated ->
    (p_change, jump_abs, p_flip, top_from, top_to, p_top, xi or None, log_z): track_pairwise's outputs from the pair marginal with both flags summed out, and
    p_flip fp32 (W-1,), the probability that the flag changes at the boundary.  log_z is track_posterior_gated's, bit for bit.  Allocates the outputs and the
    4 W C floats of workspace; nothing is read back."""
    W, C = _gated_inputs(logits, gate_logits)
    dev = logits.device
    (p_change, jump_abs, p_flip, p_top), top_from, top_to, xi_t, log_z = _pairwise_outputs(W, C, dev, xi, 4)
    ws = torch.empty(4 * max(W, 1) * C, device=dev, dtype=torch.float32)
    rc = _lib.load().sf_track_pairwise_gated(_dev(logits, 'logits'), _ld(logits) if W else C, _dev(gate_logits, 'gate_logits'), _ld(gate_logits) if W else 2, W, C,
                                             float(lam), float(mu), _dev(p_change, 'p_change'), _dev(jump_abs, 'jump_abs'), _dev(p_flip, 'p_flip'),
                                             _dev(top_from, 'top_from'), _dev(top_to, 'top_to'), _dev(p_top, 'p_top'), _dev(xi_t, 'xi') if xi else None,
                                             _dev(log_z, 'log_z'), _dev(ws, 'workspace'), _stream())
    _lib.check(rc, 'sf_track_pairwise_gated')
    return p_change, jump_abs, p_flip, top_from, top_to, p_top, xi_t, log_z


class TrackStreamState:
    """The carried state of one stream's fixed-lag read-out (sf_track_stream_push): `buf` the opaque device buffer, `rows` the rows pushed so far (host count),
    `closed` after a final push.  Its size does not depend on `rows`.  `gated`: whether the buffer has the gated layout (TrackGatedStreamState)."""
    gated = False

    def __init__(self, buf: torch.Tensor, C: int, lag: int, posterior: bool):
        self.buf, self.C, self.lag, self.posterior, self.rows, self.closed = buf, int(C), int(lag), bool(posterior), 0, False


class TrackPoolState:
    """The carried states of a pool of streams (sf_track_pool_push): `buf` uint8 (n_slots, bytes) on the device, slot i the state of one stream
    (sf_track_stream_push's layout); `rows[i]` the rows pushed into slot i so far and `closed[i]` after its final push (host counts).  `gated`: whether the slots
    have the gated layout (TrackGatedPoolState)."""
    gated = False

    def __init__(self, buf: torch.Tensor, C: int, lag: int, posterior: bool):
        self.buf, self.C, self.lag, self.posterior = buf, int(C), int(lag), bool(posterior)
        self.n_slots = int(buf.shape[0])
        self.rows, self.closed = [0] * self.n_slots, [False] * self.n_slots

    def reopen(self, slot: int):
        """Slot `slot` starts a new stream: only the host count is reset - the device state is read only when rows_done > 0."""
        self.rows[slot], self.closed[slot] = 0, False


class TrackGatedStreamState(TrackStreamState):
    """The carried state of one stream's GATED fixed-lag read-out (sf_track_stream_push_gated): TrackStreamState's fields over a buffer of
    sf_track_stream_gated_bytes(C, lag, posterior) bytes, 2C wide.  track_stream_push refuses it, track_stream_push_gated refuses a TrackStreamState."""
    gated = True


class TrackGatedPoolState(TrackPoolState):
    """The carried states of a pool of GATED streams (sf_track_pool_push_gated): TrackPoolState's fields, each slot a gated state."""
    gated = True


def _track_kind(state, gated: bool, who: str):
    """A state knows whether it is gated; a push of the other kind raises."""
    if bool(getattr(state, 'gated', False)) != gated:
        raise TypeError(f'{who}: the state is {"gated (use the *_gated push)" if not gated else "not gated (use the push without _gated)"}: the two layouts differ')


def _track_state(cls, shape, C: int, lag: int, posterior: bool, device):
    entry = 'sf_track_stream_gated_bytes' if cls.gated else 'sf_track_stream_bytes'
    nbytes = getattr(_lib.load(), entry)(int(C), int(lag), int(bool(posterior)))
    if nbytes < 0:
        _lib.check(nbytes, entry)
    return cls(torch.zeros(*shape, nbytes, device=device, dtype=torch.uint8), C, lag, posterior)


def track_stream_state(C: int, lag: int, posterior: bool, device) -> TrackStreamState:
    """A fresh stream state for C classes (2 .. 64) and a decision lag of `lag` windows (0 .. 255): sf_track_stream_bytes(C, lag, posterior) zeroed bytes on `device`."""
    return _track_state(TrackStreamState, (), C, lag, posterior, device)


def track_stream_state_gated(C: int, lag: int, posterior: bool, device) -> TrackGatedStreamState:
    """A fresh gated stream state for C classes (2 .. 32) and a decision lag of `lag` windows (0 .. 255): sf_track_stream_gated_bytes(C, lag, posterior) zeroed bytes."""
    return _track_state(TrackGatedStreamState, (), C, lag, posterior, device)


def track_pool_state(n_slots: int, C: int, lag: int, posterior: bool, device) -> TrackPoolState:
    """n_slots fresh stream states in one zeroed (n_slots, sf_track_stream_bytes(C, lag, posterior)) buffer on `device` (the size is a multiple of 16: the stride)."""
    if n_slots < 1:
        raise ValueError(f'track_pool_state: n_slots = {n_slots}')
    return _track_state(TrackPoolState, (int(n_slots),), C, lag, posterior, device)


def track_pool_state_gated(n_slots: int, C: int, lag: int, posterior: bool, device) -> TrackGatedPoolState:
    """n_slots fresh gated stream states in one zeroed (n_slots, sf_track_stream_gated_bytes(C, lag, posterior)) buffer on `device`."""
    if n_slots < 1:
        raise ValueError(f'track_pool_state_gated: n_slots = {n_slots}')
    return _track_state(TrackGatedPoolState, (int(n_slots),), C, lag, posterior, device)


TrackStreamOut = namedtuple('TrackStreamOut', 'w0 cls_raw conf_raw cls_lag conf_lag cls_tail conf_tail post_lag cls_post_lag conf_post_lag offset_mean_lag log_z')
TrackGatedStreamOut = namedtuple('TrackGatedStreamOut', TrackStreamOut._fields + ('sync_raw', 'sync_lag', 'sync_tail', 'p_sync_lag'))


def track_stream_counts(rows: int, n: int, lag: int, final: bool = False):
    """-> (w0, n_commit, n_tail) of a push of n rows onto `rows` rows: the first window it commits, how many it commits, the uncommitted tail after it."""
    done_old = max(0, rows - lag)
    done_new = rows + n if final else max(0, rows + n - lag)
    return done_old, done_new - done_old, rows + n - done_new


# the size query of each push's workspace, by the public name of the push (its C entry is 'sf_' + that name)
_TRACK_WORKSPACE_ENTRY = {'track_stream_push': 'sf_track_stream_workspace_bytes', 'track_stream_push_gated': 'sf_track_stream_gated_workspace_bytes',
                          'track_pool_push': 'sf_track_pool_workspace_bytes', 'track_pool_push_gated': 'sf_track_pool_gated_workspace_bytes'}


def _track_push_call(who: str, state, head: tuple, logits: torch.Tensor, gate_logits: Optional[torch.Tensor], lam: float, mu: float,
                     grid: Optional[torch.Tensor], final: tuple, k: int, m: int, n_z: int, post: Optional[torch.Tensor] = None) -> tuple:
    """What the four pushes share (gate_logits None: the plain chain): the input rules - logits fp32 (n, C), gate_logits fp32 (n, 2), on the state's device with unit
    column stride, with the posterior a contiguous fp32 grid (C,) - then the outputs of a push of n rows that commits k windows and leaves m in the tail (the sync
    fields for a gated state only, the posterior fields - log_z with n_z entries - with the posterior only: the others stay None), the workspace and the call of the
    C entry with `head`, the inputs, the costs, the grid, `final` and the outputs -> the outputs in TrackGatedStreamOut's field order (without w0).  Straight-line on
    purpose: a one-row push is bound by this function, not by its kernels."""
    C, dev, gated, posterior = state.C, state.buf.device, gate_logits is not None, state.posterior
    n = logits.shape[0]
    assert n == 0 or (logits.device == dev and logits.stride(1) == 1 and (not gated or (gate_logits.device == dev and gate_logits.stride(1) == 1))), \
        'logits, gate_logits: on the state\'s device, unit column stride'
    if posterior:
        assert grid is not None and grid.dtype == torch.float32 and grid.device == dev and grid.shape == (C,) and grid.is_contiguous(), f'a grid for {C} classes'
    i32 = dict(device=dev, dtype=torch.int32)
    f32 = dict(device=dev, dtype=torch.float32)
    cls_raw, conf_raw = torch.empty(n, **i32), torch.empty(n, **f32)
    cls_lag, conf_lag = torch.empty(k, **i32), torch.empty(k, **f32)
    cls_tail, conf_tail = torch.empty(m, **i32), torch.empty(m, **f32)
    sync_raw = sync_lag = sync_tail = p_sync = cls_post = conf_post = mean = log_z = None
    if gated:
        sync_raw, sync_lag, sync_tail = torch.empty(n, **f32), torch.empty(k, **i32), torch.empty(m, **i32)
    assert post is None or posterior, 'post: only with the posterior'
    if posterior:
        if post is None:
            post = torch.empty(k, C, **f32)
        assert post.dtype == torch.float32 and post.shape == (k, C) and post.device == dev and (k == 0 or post.stride(1) == 1), f'post: fp32 ({k}, {C}), unit column stride'
        cls_post, conf_post, mean = torch.empty(k, **i32), torch.empty(k, **f32), torch.empty(k, **f32)
        log_z = torch.zeros(n_z, **f32)                                             # (stays 0 for a stream that is still empty: the empty product)
        if gated:
            p_sync = torch.empty(k, **f32)
    lib = _lib.load()
    ws_entry = _TRACK_WORKSPACE_ENTRY[who]
    ws_bytes = getattr(lib, ws_entry)(C, n, int(posterior))
    if ws_bytes < 0:
        _lib.check(ws_bytes, ws_entry)
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)

    def ptr(t):
        return _dev(t, 'out') if t is not None and t.numel() else None

    ldl, g, ldp = _ld(logits) if n else C, _dev(grid, 'grid') if posterior else None, _ld(post) if posterior and k else C
    if gated:
        rc = getattr(lib, 'sf_' + who)(
            *head, ptr(logits), ldl, ptr(gate_logits), _ld(gate_logits) if n else 2, n, float(lam), float(mu), g, *final, ptr(cls_raw), ptr(conf_raw), ptr(sync_raw),
            ptr(cls_lag), ptr(sync_lag), ptr(conf_lag), ptr(post), ldp, ptr(p_sync), ptr(cls_post), ptr(conf_post), ptr(mean), ptr(cls_tail), ptr(sync_tail), ptr(conf_tail),
            ptr(log_z), _dev(ws, 'workspace'), _stream())
    else:
        rc = getattr(lib, 'sf_' + who)(
            *head, ptr(logits), ldl, n, float(lam), g, *final, ptr(cls_raw), ptr(conf_raw), ptr(cls_lag), ptr(conf_lag), ptr(post), ldp, ptr(cls_post), ptr(conf_post),
            ptr(mean), ptr(cls_tail), ptr(conf_tail), ptr(log_z), _dev(ws, 'workspace'), _stream())
    if rc:
        _lib.check(rc, 'sf_' + who)
    return cls_raw, conf_raw, cls_lag, conf_lag, cls_tail, conf_tail, post, cls_post, conf_post, mean, log_z, sync_raw, sync_lag, sync_tail, p_sync


def _track_stream_push(who: str, state: TrackStreamState, logits: torch.Tensor, gate_logits: Optional[torch.Tensor], lam: float, mu: float,
                       grid: Optional[torch.Tensor], final: bool):
    """track_stream_push (gate_logits None) and track_stream_push_gated: `who` is the public name."""
    gated = gate_logits is not None
    _track_kind(state, gated, who)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == state.C, f'{who}: logits {tuple(logits.shape)} for a stream of {state.C} classes'
    n = logits.shape[0]
    assert not gated or (gate_logits.dtype == torch.float32 and gate_logits.shape == (n, 2)), f'{who}: gate logits of {tuple(gate_logits.shape)} for {n} rows'
    if state.closed:
        raise RuntimeError(f'{who}: the stream was closed by a final push')
    w0, k, m = track_stream_counts(state.rows, n, state.lag, final)
    head = (_dev(state.buf, 'state'), state.C, state.lag, int(state.posterior), state.rows)
    o = _track_push_call(who, state, head, logits, gate_logits, lam, mu, grid, (int(bool(final)),), k, m, 1)
    state.rows += n
    state.closed = bool(final)
    return TrackGatedStreamOut(w0, *o) if gated else TrackStreamOut(w0, *o[:11])


def track_stream_push(state: TrackStreamState, logits: torch.Tensor, lam: float, grid: Optional[torch.Tensor] = None, final: bool = False) -> TrackStreamOut:
    """Fixed-lag read-out of the next n rows of a stream (sf_track_stream_push): logits fp32 (n, C) on the state's device with unit column stride (n = 0 allowed),
    rows in time order after the state.rows pushed before; grid fp32 (C,) when the state was made with posterior ->
    TrackStreamOut(w0, cls_raw (n,), conf_raw (n,), cls_lag (k,), conf_lag (k,), cls_tail (m,), conf_tail (m,), post_lag (k, C), cls_post_lag, conf_post_lag,
    offset_mean_lag (k,), log_z (1,)): windows w0 .. w0 + k - 1 are committed by this push (those whose row w + lag arrived: cls_lag[i] is the class of window
    w0 + i on the Viterbi path of rows 0 .. w0 + i + lag, never revised), the tail is the path of everything pushed so far on the m = min(lag, rows) windows not yet
    committed (cls_tail[-1]: the current offset).  final=True commits the tail from the whole prefix and closes the state.  The posterior fields are None without
    posterior.  Output sizes are host arithmetic; nothing is read back or synchronised, the state advances on the device in stream order."""
    return _track_stream_push('track_stream_push', state, logits, None, lam, 0.0, grid, final)


def track_stream_push_gated(state: TrackGatedStreamState, logits: torch.Tensor, gate_logits: torch.Tensor, lam: float, mu: float, grid: Optional[torch.Tensor] = None,
                            final: bool = False) -> TrackGatedStreamOut:
    """Gated fixed-lag read-out of the next n rows of a stream (sf_track_stream_push_gated): logits fp32 (n, C) and gate_logits fp32 (n, 2) of the same
    windows, on the state's device with unit column stride (n = 0 allowed) -> TrackGatedStreamOut: TrackStreamOut's fields read from the chain over (offset class,
    synchronizable flag) - (cls_lag[i], sync_lag[i]) is window w0 + i on ops.track_decode_gated's path of rows 0 .. w0 + i + lag, post_lag / p_sync_lag[i] its row of
    ops.track_posterior_gated on that prefix - plus sync_raw (n,) fp32, sync_lag (k,) int32, sync_tail (m,) int32 and p_sync_lag (k,) fp32 (None without posterior).
    Counts, final and the no-read-back rule are track_stream_push's."""
    return _track_stream_push('track_stream_push_gated', state, logits, gate_logits, lam, mu, grid, final)


TRACK_POOL_ROW = 8                       # int64 per descriptor row: slot, rows_done, n, row0, final, commit0, tail0, unused
TRACK_POOL_MAX_ACTIVE = 4096
TrackPoolPlan = namedtuple('TrackPoolPlan', 'table total_rows total_commit total_tail blocks')


def track_pool_plan(rows, counts, lag: int, final, slots=None) -> TrackPoolPlan:
    """The descriptor table of one pool push (sf_track_pool_push), pure host arithmetic: entry i pushes counts[i] rows onto a stream that holds rows[i], final[i]
    truthy closes it, slots[i] (default i) names its state -> TrackPoolPlan(table int64 (n, 8) on the host: slot, rows_done, n, row0, final, commit0, tail0, 0;
    total_rows, total_commit, total_tail: the sizes of the packed blocks; blocks: per entry (w0, n_commit, n_tail) = track_stream_counts).  The rows, the
    committed blocks and the tails of the entries lie back to back in table order: row0 / commit0 / tail0 are the running sums."""
    rows, counts, final = [int(r) for r in rows], [int(c) for c in counts], [bool(f) for f in final]
    slots = list(range(len(rows))) if slots is None else [int(x) for x in slots]
    if not (len(rows) == len(counts) == len(final) == len(slots)):
        raise ValueError(f'track_pool_plan: {len(rows)} row counts, {len(counts)} push sizes, {len(final)} final flags, {len(slots)} slots')
    if min(rows + counts + [int(lag)], default=0) < 0:
        raise ValueError('track_pool_plan: negative rows, counts or lag')
    row0 = commit0 = tail0 = 0
    table, blocks = [], []
    for slot, r, n, f in zip(slots, rows, counts, final):
        w0, k, m = track_stream_counts(r, n, lag, f)
        table.append((slot, r, n, row0, int(f), commit0, tail0, 0))
        blocks.append((w0, k, m))
        row0, commit0, tail0 = row0 + n, commit0 + k, tail0 + m
    table = torch.tensor(table, dtype=torch.int64).reshape(len(rows), TRACK_POOL_ROW)
    return TrackPoolPlan(table, row0, commit0, tail0, blocks)


def _track_pool_table(who: str, state: TrackPoolState, slots, counts, final, total: int):
    """The host rules of a pool push and its descriptor table -> (slots, counts, final as a set, plan, the pinned host table, its device copy): distinct open slots of
    the state, counts that add up to the `total` rows, track_pool_plan, one non-blocking upload from a FRESH pinned tensor (see track_pool_push)."""
    slots, counts, final = [int(x) for x in slots], [int(x) for x in counts], {int(x) for x in final}
    if len(slots) != len(counts) or not 1 <= len(slots) <= TRACK_POOL_MAX_ACTIVE:
        raise ValueError(f'{who}: {len(slots)} slots, {len(counts)} counts (1 .. {TRACK_POOL_MAX_ACTIVE} streams in one push)')
    if len(set(slots)) != len(slots) or not all(0 <= x < state.n_slots for x in slots) or not final <= set(slots):
        raise ValueError(f'{who}: slots {slots} (final {sorted(final)}): distinct, below {state.n_slots}, the final ones among them')
    if any(state.closed[x] for x in slots):
        raise RuntimeError(f'{who}: slots {[x for x in slots if state.closed[x]]} were closed by a final push (reopen them)')
    if min(counts) < 0 or sum(counts) != total:
        raise ValueError(f'{who}: counts {counts} for {total} rows of logits')
    plan = track_pool_plan([state.rows[x] for x in slots], counts, state.lag, [x in final for x in slots], slots)
    host = torch.empty(len(slots), TRACK_POOL_ROW, dtype=torch.int64, pin_memory=True)
    host.copy_(plan.table)
    return slots, counts, final, plan, host, host.to(state.buf.device, non_blocking=True)


def _track_pool_push(who: str, state: TrackPoolState, slots, logits: torch.Tensor, gate_logits: Optional[torch.Tensor], counts, lam: float, mu: float,
                     grid: Optional[torch.Tensor], final, post: Optional[torch.Tensor]) -> list:
    """track_pool_push (gate_logits None) and track_pool_push_gated: `who` is the public name."""
    gated = gate_logits is not None
    _track_kind(state, gated, who)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == state.C, f'{who}: logits {tuple(logits.shape)} for streams of {state.C} classes'
    total = logits.shape[0]
    assert not gated or (gate_logits.dtype == torch.float32 and gate_logits.shape == (total, 2)), f'{who}: gate logits of {tuple(gate_logits.shape)} for {total} rows'
    slots, counts, final, plan, host, table = _track_pool_table(who, state, slots, counts, final, total)
    head = (_dev(state.buf, 'states'), state.buf.stride(0), state.n_slots, state.C, state.lag, int(state.posterior), host.data_ptr(), _dev(table, 'table'), len(slots))
    o = _track_push_call(who, state, head, logits, gate_logits, lam, mu, grid, (), plan.total_commit, plan.total_tail, len(slots), post)
    # one result per slot: views into the packed outputs (one split per field, not one slice per slot and field); the fields' sizes in TrackGatedStreamOut's order
    ns, ks, ms = counts, [b[1] for b in plan.blocks], [b[2] for b in plan.blocks]
    sizes = (ns, ns, ks, ks, ms, ms, ks, ks, ks, ks, 1, ns, ks, ms, ks)
    none = [None] * len(slots)
    out, width = (TrackGatedStreamOut, 15) if gated else (TrackStreamOut, 11)
    fields = [none if t is None else t.split(size) for t, size in zip(o[:width], sizes)]
    outs = [out(b[0], *views) for b, views in zip(plan.blocks, zip(*fields))]
    for slot, n in zip(slots, ns):
        state.rows[slot] += n
        state.closed[slot] = slot in final
    return outs


def track_pool_push(state: TrackPoolState, slots, logits: torch.Tensor, counts, lam: float, grid: Optional[torch.Tensor] = None, final=(),
                    post: Optional[torch.Tensor] = None) -> list:
    """One push for many streams (sf_track_pool_push): logits fp32 (total, C) on the state's device with unit column stride, the new rows of all named streams
    packed in the order of `slots` - counts[i] rows (0 allowed) belong to the stream in slots[i]; `final`: the slots this push closes -> one TrackStreamOut per
    slot, views into the packed outputs, each equal bit for bit to track_stream_push on that stream alone (log_z: its own (1,) view).  The number of launches and
    of allocations does not depend on len(slots).  The descriptor table is built on the host (track_pool_plan), copied into a FRESH PINNED tensor and uploaded
    with one non-blocking copy on the current stream: no buffer is shared between two pushes, so a later push cannot race the upload (torch's pinned-memory
    allocator keeps the block until the copy has run).  Nothing is read back or synchronised.  `post` (posterior only), if given, is written instead of a fresh
    tensor: fp32 (total_commit, C) - track_pool_plan's count - with unit column stride and any row stride >= C."""
    return _track_pool_push('track_pool_push', state, slots, logits, None, counts, lam, 0.0, grid, final, post)


def track_pool_push_gated(state: TrackGatedPoolState, slots, logits: torch.Tensor, gate_logits: torch.Tensor, counts, lam: float, mu: float,
                          grid: Optional[torch.Tensor] = None, final=(), post: Optional[torch.Tensor] = None) -> list:
    """One gated push for many streams (sf_track_pool_push_gated): track_pool_push's arguments plus gate_logits fp32 (total, 2), packed like logits (the gate rows of a
    stream are the rows of its offset logits), and mu -> one TrackGatedStreamOut per slot, views into the packed outputs, each equal bit for bit to
    track_stream_push_gated on that stream alone.  The table, its upload and every host rule are track_pool_push's."""
    return _track_pool_push('track_pool_push_gated', state, slots, logits, gate_logits, counts, lam, mu, grid, final, post)


def _ingest_tables(frame_table: torch.Tensor, **tables):
    """Checks frame_table (int32, contiguous) and the filter tables name=(first int32 (224,), weights fp32 (224, taps)), all contiguous; returns their launcher
    arguments in order: (first, weights, taps) per table."""
    firsts, weights = [f for f, _ in tables.values()], [w for _, w in tables.values()]
    assert frame_table.dtype == torch.int32 and all(t.dtype == torch.int32 and t.shape == (INGEST_OUT,) for t in firsts)
    assert all(t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == INGEST_OUT for t in weights)
    assert all(t.is_contiguous() for t in (frame_table, *firsts, *weights))
    return [a for k, (f, w) in tables.items() for a in (_dev(f, f'{k}_first'), _dev(w, f'{k}_w'), w.shape[1])]


def _ingest_out(out: Optional[torch.Tensor], T_out: int, device) -> torch.Tensor:
    if out is None:
        out = torch.empty(T_out, 3, INGEST_OUT, INGEST_OUT, device=device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.shape == (T_out, 3, INGEST_OUT, INGEST_OUT) and out.is_contiguous()
    return out


def _ingest_chunks(entry: str, head, frame_table: torch.Tensor, tail, out: Optional[torch.Tensor], device) -> torch.Tensor:
    """The library's `entry`(*head, frame_table, *tail, out, n, stream) for every 65535 output frames: what one launch takes."""
    T_out = frame_table.numel()
    out = _ingest_out(out, T_out, device)
    for t0 in range(0, max(T_out, 1), 65535):
        _lib.check(getattr(_lib.load(), entry)(*head, _dev(frame_table[t0:], 'frame_table'), *tail, _dev(out[t0:], 'out'), min(65535, T_out - t0), _stream()), entry)
    return out


def _ingest_rgb_source(who: str, raw: torch.Tensor, channels_last: bool, fields: bool = False):
    """The RGB frames of `who` -> the launcher's (frame, channel, row, column strides, n_src, H, W); fields: H has to hold two of them."""
    if raw.dim() != 4 or raw.dtype != torch.uint8 or raw.shape[3 if channels_last else 1] != 3:
        raise ValueError(f'{who}: expected uint8 frames (n, 3, H, W) or channels_last (n, H, W, 3), got {raw.dtype} {tuple(raw.shape)}')
    (H, W), (sf, sc, sy, sx) = ((raw.shape[1], raw.shape[2]), (raw.stride(i) for i in (0, 3, 1, 2))) if channels_last else \
        ((raw.shape[2], raw.shape[3]), raw.stride())
    if fields and (H < 2 or H % 2):
        raise ValueError(f'{who}: H = {H}: two fields take an even H')
    assert min(sf, sc, sy) >= 0 and sx >= 1, f'{who}: negative strides'
    return sf, sc, sy, sx, raw.shape[0], H, W


def _ingest_420_source(who: str, raw: torch.Tensor, pix_fmt: str, semi: str, planar: str, dtypes):
    """The 4:2:0 frames (n_src, 3 H / 2, W) of `who`, in its semi-planar format (H luma rows, then H / 2 rows of interleaved U V) or its planar one (I420 order) ->
    the launcher's (frame stride, row stride, U offset, V offset, chroma row stride, chroma column stride) in BYTES, then (n_src, H, W)."""
    b = dtypes[0].itemsize
    if pix_fmt not in (semi, planar):
        raise ValueError(f"{who}: pix_fmt = {pix_fmt!r} ('{semi}' or '{planar}')")
    if raw.dim() != 3 or raw.dtype not in dtypes or raw.shape[1] % 3 or raw.shape[2] % 2 or raw.shape[1] == 0 or raw.shape[2] == 0:
        raise ValueError(f'{who}: expected uint{8 * b} frames (n, 3 H / 2, W) with even H and W, got {raw.dtype} {tuple(raw.shape)}')
    n_src, H, W = raw.shape[0], raw.shape[1] // 3 * 2, raw.shape[2]
    sf, sy, sx = raw.stride()
    if sx != 1 or sf < 0 or (sy != W if pix_fmt == planar else sy < W):
        raise ValueError(f'{who}: {pix_fmt} frames with strides {tuple(raw.stride())}: unit column stride and '
                         f'{"contiguous rows" if pix_fmt == planar else "a row stride of at least W"} expected')
    u_off, v_off, csy, csx = (sy * H, sy * H + 1, sy, 2) if pix_fmt == semi else (H * W, H * W + (H // 2) * (W // 2), W // 2, 1)
    return [b * v for v in (sf, sy, u_off, v_off, csy, csx)], (n_src, H, W)


def _ingest_plane_source(who: str, raw: torch.Tensor, L, fields: bool = False):
    """The frames of `who` against the ingest.PlaneLayout L (ValueError: a dtype that does not hold L.bytes_per_sample bytes, a plane that reaches outside the tensor;
    fields: a layout that does not hold two of them) -> the launcher's arguments between raw and the table."""
    if raw.dim() < 2 or raw.dtype not in ((torch.uint8,) if L.bytes_per_sample == 1 else (torch.uint16, torch.int16)):
        raise ValueError(f'{who}: expected {"uint8" if L.bytes_per_sample == 1 else "uint16"} frames (n, ...) for samples of {L.bytes_per_sample} '
                         f'byte(s), got {raw.dtype} {tuple(raw.shape)}')
    n_src, b = raw.shape[0], L.bytes_per_sample
    if min(L) < 0 or min(L.H, L.W, L.Hc, L.Wc) < 1 or min(L.stride_col, L.stride_ccol) < b:
        raise ValueError(f'{who}: {L}: negative entries, an empty plane or a column stride below a sample')
    if fields and (L.H % 2 or L.Hc != L.H):
        raise ValueError(f'{who}: {L}: two fields take an even H and chroma planes of H rows (4:2:2, 4:4:4)')
    # the last byte any plane reaches against the bytes the tensor spans from its first element (strides >= 0 for a frame tensor; a negative one is refused)
    if any(s < 0 for s in raw.stride()):
        raise ValueError(f'{who}: frames with strides {tuple(raw.stride())}')
    span = (1 + sum((n - 1) * s for n, s in zip(raw.shape, raw.stride()))) * raw.element_size() if raw.numel() else 0
    ends = [off + (h - 1) * sr + (w - 1) * sc + b for off, h, sr, w, sc in ((L.y_off, L.H, L.stride_row, L.W, L.stride_col),
                                                                              (L.u_off, L.Hc, L.stride_crow, L.Wc, L.stride_ccol),
                                                                              (L.v_off, L.Hc, L.stride_crow, L.Wc, L.stride_ccol))]
    if n_src < 1 or (n_src - 1) * L.stride_frame + max(ends) > span:
        raise ValueError(f'{who}: {L} reaches byte {(n_src - 1) * L.stride_frame + max(ends)} of {n_src} frames that span {span} bytes '
                         f'({raw.dtype} {tuple(raw.shape)}, strides {tuple(raw.stride())})')
    return (b, L.stride_frame, L.y_off, L.stride_row, L.stride_col, L.u_off, L.v_off, L.stride_crow, L.stride_ccol, L.shift, n_src, L.H, L.W, L.Hc, L.Wc)


def _ingest_csc(who: str, csc):
    """csc, a tensor or a sequence of 12 floats -> the float[12] the launchers read (their argument is its address: the caller holds it over the call)."""
    csc = [float(v) for v in (csc.reshape(-1).tolist() if isinstance(csc, torch.Tensor) else csc)]
    assert len(csc) == 12, f'{who}: csc is 9 matrix entries and 3 offsets'
    return (C.c_float * 12)(*csc)


def ingest_video(raw: torch.Tensor, channels_last: bool, frame_table: torch.Tensor, y_first: torch.Tensor, y_w: torch.Tensor, x_first: torch.Tensor,
                 x_w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frame pick + antialiased resize + crop in one launch (sf_ingest_video): raw uint8 on the device, (n_src, 3, H, W) or - channels_last - (n_src, H, W, 3),
    any strides (a view is read in place); frame_table int32 (T_out,) of source frame indices inside [0, n_src); y_first / x_first int32 (224,) and
    y_w / x_w fp32 (224, taps) contiguous: the filter tables already sliced to the crop -> uint8 (T_out, 3, 224, 224)."""
    geom = _ingest_rgb_source('ingest_video', raw, channels_last)
    head, tabs = (_dev(raw, 'raw'), *geom), _ingest_tables(frame_table, y=(y_first, y_w), x=(x_first, x_w))
    return _ingest_chunks('sf_ingest_video', head, frame_table, tabs, out, raw.device)


def ingest_video_yuv(raw: torch.Tensor, pix_fmt: str, frame_table: torch.Tensor, y_first: torch.Tensor, y_w: torch.Tensor, x_first: torch.Tensor, x_w: torch.Tensor,
                     cy_first: torch.Tensor, cy_w: torch.Tensor, cx_first: torch.Tensor, cx_w: torch.Tensor, csc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video for 8-bit YUV 4:2:0 frames (sf_ingest_video_yuv): the three planes are resized, the colour matrix runs on the 224 x 224 result.  raw uint8
    (n_src, 3 H / 2, W) on the device, H and W even, any frame stride; pix_fmt 'nv12' (H luma rows, then H / 2 rows of interleaved U V; any row stride >= W, so a
    view into a pitched decoder surface is read in place) or 'yuv420p' (I420 as PyAV's to_ndarray gives it: H W luma bytes, then the U plane, then the V plane,
    H / 2 x W / 2 each; contiguous rows).  y_* / x_*: the luma tables of ingest_video; cy_* / cx_*: the chroma tables (H / 2 -> Hr, W / 2 -> Wr), sliced at the
    same crop origin; csc: 12 floats, the matrix row-major (rows R, G, B; columns Y, U, V) then the three offsets (ingest.csc_matrix) -> uint8 (T_out, 3, 224, 224)."""
    strides, size = _ingest_420_source('ingest_video_yuv', raw, pix_fmt, 'nv12', 'yuv420p', (torch.uint8,))
    csc_c = _ingest_csc('ingest_video_yuv', csc)
    head, tabs = (_dev(raw, 'raw'), *strides, *size), _ingest_tables(frame_table, y=(y_first, y_w), x=(x_first, x_w), cy=(cy_first, cy_w), cx=(cx_first, cx_w))
    return _ingest_chunks('sf_ingest_video_yuv', head, frame_table, (*tabs, C.addressof(csc_c)), out, raw.device)


_YUV16_SHIFT = {'p010': 6, 'yuv420p10le': 0}


def ingest_video_yuv16(raw: torch.Tensor, pix_fmt: str, frame_table: torch.Tensor, y_first: torch.Tensor, y_w: torch.Tensor, x_first: torch.Tensor, x_w: torch.Tensor,
                       cy_first: torch.Tensor, cy_w: torch.Tensor, cx_first: torch.Tensor, cx_w: torch.Tensor, csc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video_yuv for 10-bit YUV 4:2:0 frames in 16-bit samples (sf_ingest_video_yuv16).  raw uint16 (or int16, read as the same bits) (n_src, 3 H / 2, W) on
    the device, H and W even, any frame stride; pix_fmt 'p010' (H luma rows, then H / 2 rows of interleaved U V, the sample in the high 10 bits; any row stride >= W
    elements, so a view into a pitched decoder surface is read in place) or 'yuv420p10le' (I420 order, the sample in the low 10 bits; contiguous rows).  The sample is
    (word >> shift) & 1023, so stray bits are dropped.  Tables as for ingest_video_yuv; csc: 12 floats on the 10-bit scale (ingest.csc_matrix(bit_depth=10)) ->
    uint8 (T_out, 3, 224, 224)."""
    strides, size = _ingest_420_source('ingest_video_yuv16', raw, pix_fmt, 'p010', 'yuv420p10le', (torch.uint16, torch.int16))
    csc_c = _ingest_csc('ingest_video_yuv16', csc)
    head = (_dev(raw, 'raw'), *strides, _YUV16_SHIFT[pix_fmt], *size)
    tabs = _ingest_tables(frame_table, y=(y_first, y_w), x=(x_first, x_w), cy=(cy_first, cy_w), cx=(cx_first, cx_w))
    return _ingest_chunks('sf_ingest_video_yuv16', head, frame_table, (*tabs, C.addressof(csc_c)), out, raw.device)


def ingest_video_planes(raw: torch.Tensor, layout, frame_table: torch.Tensor, y_first: torch.Tensor, y_w: torch.Tensor, x_first: torch.Tensor, x_w: torch.Tensor,
                        cy_first: torch.Tensor, cy_w: torch.Tensor, cx_first: torch.Tensor, cx_w: torch.Tensor, csc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The general YUV ingest (sf_ingest_video_yuv_planes): raw uint8, or uint16 / int16 (the same bits), on the device, frames along dim 0, any shape
    behind it; layout: an ingest.PlaneLayout (ingest.plane_layout for the named formats, or written out: 4:4:4 planar is Hc = H, Wc = W with the luma tables for
    chroma) saying in BYTES where the three planes of a frame lie and how many bytes a sample has.  y_* / x_*: the luma tables (H -> Hr, W -> Wr); cy_* / cx_*: the
    chroma tables (Hc -> Hr, Wc -> Wr), sliced at the same crop origin; csc: 12 floats on the samples' own scale -> uint8 (T_out, 3, 224, 224).  ValueError when the
    dtype does not hold layout.bytes_per_sample bytes or when a plane of the layout reaches outside the tensor; what the launcher refuses is a RuntimeError."""
    geom = _ingest_plane_source('ingest_video_planes', raw, layout)
    csc_c = _ingest_csc('ingest_video_planes', csc)
    head, tabs = (_dev(raw, 'raw'), *geom), _ingest_tables(frame_table, y=(y_first, y_w), x=(x_first, x_w), cy=(cy_first, cy_w), cx=(cx_first, cx_w))
    return _ingest_chunks('sf_ingest_video_yuv_planes', head, frame_table, (*tabs, C.addressof(csc_c)), out, raw.device)


def _field_pairs(what: str, **pairs):
    """name=((first0, w0), (first1, w1)): the vertical tables of the fields of parity 0 and parity 1 share one tap count (ValueError otherwise)."""
    for k, (t0, t1) in pairs.items():
        if t0[1].shape != t1[1].shape:
            raise ValueError(f'{what}: the {k} tables of the two parities have {t0[1].shape[-1]} and {t1[1].shape[-1]} taps; one tap count serves both')


def _field_tables(field_table: torch.Tensor, **pairs):
    """The launcher arguments of the field entries' vertical tables, name=((first0, w0), (first1, w1)) -> (first0, w0, first1, w1, taps) per name, after
    _ingest_tables' checks on all of them."""
    args = []
    for k, (t0, t1) in pairs.items():
        a = _ingest_tables(field_table, **{f'{k}0': t0, f'{k}1': t1})
        args += [a[0], a[1], a[3], a[4], a[2]]
    return args


def ingest_video_fields(raw: torch.Tensor, channels_last: bool, field_table: torch.Tensor, y_tables, x_first: torch.Tensor, x_w: torch.Tensor, bottom_first: bool,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video on an interlaced recording (sf_ingest_video_fields): raw as for ingest_video, H even; field_table int32 (T_out,) of FIELD indices
    inside [0, 2 n_src) - field f is rows p, p + 2, .. of frame f >> 1, p = (f & 1) ^ bottom_first; y_tables = ((first0, w0), (first1, w1)): the vertical tables of
    the fields of parity 0 and 1 (H / 2 rows -> Hr, shift 0.25 - p / 2, sliced to the crop), one tap count; x_first / x_w as for ingest_video -> uint8
    (T_out, 3, 224, 224): every output frame is one field, resized on its own."""
    geom = _ingest_rgb_source('ingest_video_fields', raw, channels_last, fields=True)
    _field_pairs('ingest_video_fields', y=y_tables)
    head = (_dev(raw, 'raw'), *geom)
    tabs = _field_tables(field_table, y=y_tables) + _ingest_tables(field_table, x=(x_first, x_w))
    return _ingest_chunks('sf_ingest_video_fields', head, field_table, (*tabs, int(bool(bottom_first))), out, raw.device)


def ingest_video_planes_fields(raw: torch.Tensor, layout, field_table: torch.Tensor, y_tables, x_first: torch.Tensor, x_w: torch.Tensor, cy_tables,
                               cx_first: torch.Tensor, cx_w: torch.Tensor, csc, bottom_first: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video_planes on an interlaced recording (sf_ingest_video_yuv_planes_fields): raw and layout as there, with layout.Hc == layout.H even (4:2:2,
    4:4:4: full vertical chroma resolution); field_table, y_tables and bottom_first as for ingest_video_fields; cy_tables: the chroma planes' pair of vertical tables
    (for 4:2:2 the luma pair); the horizontal tables and csc as for ingest_video_planes -> uint8 (T_out, 3, 224, 224)."""
    geom = _ingest_plane_source('ingest_video_planes_fields', raw, layout, fields=True)
    csc_c = _ingest_csc('ingest_video_planes_fields', csc)
    _field_pairs('ingest_video_planes_fields', y=y_tables, cy=cy_tables)
    head = (_dev(raw, 'raw'), *geom)
    ytabs, cytabs = _field_tables(field_table, y=y_tables), _field_tables(field_table, cy=cy_tables)
    xtabs, cxtabs = _ingest_tables(field_table, x=(x_first, x_w)), _ingest_tables(field_table, cx=(cx_first, cx_w))
    tail = (*ytabs, *xtabs, *cytabs, *cxtabs, C.addressof(csc_c), int(bool(bottom_first)))
    return _ingest_chunks('sf_ingest_video_yuv_planes_fields', head, field_table, tail, out, raw.device)


def _ingest_v210_source(who: str, raw: torch.Tensor, W: int, fields: bool = False):
    """The v210 frames of `who` -> the launcher's (frame stride, row stride) in BYTES, then (n_src, H, W).  ValueError: a host tensor, another dtype or rank, odd W,
    rows shorter than the whole groups of W pixels, a column stride other than 1, a negative stride; fields: an odd H."""
    W = int(W)
    if raw.dim() != 3 or raw.dtype not in (torch.int32, torch.uint32):
        raise ValueError(f'{who}: expected int32 or uint32 v210 frames (n, H, words per row), got {raw.dtype} {tuple(raw.shape)}')
    if W < 2 or W % 2:
        raise ValueError(f'{who}: W = {W}: v210 takes an even W')
    need = 4 * -(-W // 6)
    if raw.shape[2] < need:
        raise ValueError(f'{who}: rows of {raw.shape[2]} words, a v210 row of {W} pixels has {need} (four per six pixels, whole groups)')
    n_src, H = raw.shape[0], raw.shape[1]
    sf, sy, sx = raw.stride()
    if sx != 1 or sf < 0 or sy < 0:
        raise ValueError(f'{who}: v210 frames with strides {tuple(raw.stride())}: unit column stride and non-negative frame and row strides expected')
    if fields and (H < 2 or H % 2):
        raise ValueError(f'{who}: H = {H}: two fields take an even H')
    if raw.device.type == 'cpu':                                               # (last: everything above is checked without a device)
        raise ValueError(f'{who}: raw frames on the host: the launcher reads device memory')
    return 4 * sf, 4 * sy, n_src, H, W


def ingest_video_v210(raw: torch.Tensor, W: int, frame_table: torch.Tensor, y_first: torch.Tensor, y_w: torch.Tensor, x_first: torch.Tensor, x_w: torch.Tensor,
                      cx_first: torch.Tensor, cx_w: torch.Tensor, csc, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video_planes for v210 frames (sf_ingest_video_v210): 10-bit 4:2:2 as SDI capture hands it out, the fields Cb Y Cr Y .. of a row three to a
    32-bit word.  raw int32 or uint32 (the same bits) (n_src, H, Pw) on the device, unit stride along a row, any row stride of at least 4 ceil(W / 6) words (a pitched
    capture surface is read in place; ingest.v210_row_words), any non-negative frame stride; W: the picture's width, even.  Padding words, the unused fields of a last
    partial group and bits 30 - 31 never reach the output.  The tables as for ingest_video_planes on a 4:2:2 format - the chroma rows take the luma vertical tables, so
    there are no cy tables; csc: 12 floats on the 10-bit scale -> uint8 (T_out, 3, 224, 224), bit for bit what ingest_video_planes gives for the same samples as
    yuv422p10le.  ValueError on a host tensor, another dtype or rank, Pw below 4 ceil(W / 6), odd W, a negative stride; what the launcher refuses is a RuntimeError."""
    geom = _ingest_v210_source('ingest_video_v210', raw, W)
    csc_c = _ingest_csc('ingest_video_v210', csc)
    head, tabs = (_dev(raw, 'raw'), *geom), _ingest_tables(frame_table, y=(y_first, y_w), x=(x_first, x_w), cx=(cx_first, cx_w))
    return _ingest_chunks('sf_ingest_video_v210', head, frame_table, (*tabs, C.addressof(csc_c)), out, raw.device)


def ingest_video_v210_fields(raw: torch.Tensor, W: int, field_table: torch.Tensor, y_tables, x_first: torch.Tensor, x_w: torch.Tensor, cx_first: torch.Tensor,
                             cx_w: torch.Tensor, csc, bottom_first: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ingest_video_v210 on an interlaced recording (sf_ingest_video_v210_fields): raw and W as there with H even; field_table, y_tables and bottom_first as for
    ingest_video_fields (luma and chroma rows share the pair of vertical tables) -> uint8 (T_out, 3, 224, 224), every output frame one field."""
    geom = _ingest_v210_source('ingest_video_v210_fields', raw, W, fields=True)
    csc_c = _ingest_csc('ingest_video_v210_fields', csc)
    _field_pairs('ingest_video_v210_fields', y=y_tables)
    tabs = _field_tables(field_table, y=y_tables) + _ingest_tables(field_table, x=(x_first, x_w), cx=(cx_first, cx_w))
    tail = (*tabs, C.addressof(csc_c), int(bool(bottom_first)))
    return _ingest_chunks('sf_ingest_video_v210_fields', (_dev(raw, 'raw'), *geom), field_table, tail, out, raw.device)


SF_I16 = 4


def resample_wave(x: torch.Tensor, kernel: torch.Tensor, o: int, width: int, len_out: Optional[int] = None) -> torch.Tensor:
    """Polyphase resampler (sf_resample_wave): x fp32 or int16 (scaled by 1 / 32768) on the device, (len,) or (ch, len) with ch <= 8 averaged to mono and a unit
    sample stride; kernel fp32 (n, 2 width + o) contiguous (ingest.resample_kernel) -> fp32 (ceil(n len / o),), or its first len_out samples."""
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise ValueError(f'resample_wave: expected an fp32 or int16 wave (len,) or (ch, len), got {x.dtype} {tuple(x.shape)}')
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    ch, n_in = x.shape
    n, taps = kernel.shape
    assert kernel.dtype == torch.float32 and kernel.is_contiguous() and taps == 2 * width + o
    full = -(-n * n_in // o)
    len_out = full if len_out is None else int(len_out)
    y = torch.empty(len_out, device=x.device, dtype=torch.float32)
    rc = _lib.load().sf_resample_wave(_dev(x, 'x'), SF_F32 if x.dtype == torch.float32 else SF_I16, ch, x.stride(0) if ch > 1 else max(n_in, 1), n_in,
                                      _dev(kernel, 'kernel'), n, taps, o, width, _dev(y, 'y'), len_out, _stream())
    _lib.check(rc, 'sf_resample_wave')
    return y


SF_I32 = 5
MIX_MAX_CH, MIX_MAX_P, MIX_MAX_FLOATS, MIX_TILE = 16, 8, 16384, 256      # sf_resample_wave_mix: channels, programmes per launch, floats of LDS for the mixed rows
_MIX_DT = {torch.float32: SF_F32, torch.int16: SF_I16, torch.int32: SF_I32}


def resample_mix_span(n: int, o: int, taps: int) -> int:
    """Input samples one tile of 256 outputs may span (sf_resample_wave_mix stages them per programme): ((255 // n) + 1) o + taps."""
    return ((MIX_TILE - 1) // n + 1) * o + taps


def resample_wave_mix(x: torch.Tensor, mix: torch.Tensor, kernel: torch.Tensor, o: int, width: int, interleaved: bool = False,
                      len_out: Optional[int] = None) -> torch.Tensor:
    """The polyphase resampler for several programmes of one multi-channel wave (sf_resample_wave_mix): x fp32, int16 (scaled by 2^-15) or int32 (2^-31)
    on the device, (ch, len), or (len, ch) when `interleaved`, ch <= 16, any strided 2-D view with positive strides (anything else is copied once); mix fp32 (P, ch):
    programme p is sum_c mix[p, c] x[c]; kernel fp32 (n, 2 width + o) contiguous (ingest.resample_kernel) -> fp32 (P, ceil(n len / o)), or its first len_out
    columns.  More than 8 programmes, or more than the LDS limit holds (P * resample_mix_span <= 16384), go in several launches."""
    if x.dim() != 2 or x.dtype not in _MIX_DT or mix.dim() != 2 or mix.dtype != torch.float32:
        raise ValueError(f'resample_wave_mix: expected an fp32, int16 or int32 wave (ch, len) / (len, ch) and an fp32 mix (P, ch), got {x.dtype} {tuple(x.shape)} and '
                         f'{mix.dtype} {tuple(mix.shape)}')
    if interleaved:
        x = x.t()
    ch, n_in = x.shape
    P = mix.shape[0]
    if not 1 <= ch <= MIX_MAX_CH or mix.shape[1] != ch or P < 1:
        raise ValueError(f'resample_wave_mix: {ch} channels (1 .. {MIX_MAX_CH}) with a mix of {tuple(mix.shape)}')
    xp, mp, kp = _dev(x, 'x'), _dev(mix, 'mix'), _dev(kernel, 'kernel')
    if (ch > 1 and x.stride(0) < 1) or (n_in > 1 and x.stride(1) < 1):           # a layout two positive strides cannot express: one contiguous copy
        x = x.contiguous()
        xp = x.data_ptr()
    if not mix.is_contiguous():
        mix = mix.contiguous()
        mp = mix.data_ptr()
    n, taps = kernel.shape
    assert kernel.dtype == torch.float32 and kernel.is_contiguous() and taps == 2 * width + o
    per = min(MIX_MAX_P, MIX_MAX_FLOATS // resample_mix_span(n, o, taps))
    if per < 1:
        raise ValueError(f'resample_wave_mix: a tile spans {resample_mix_span(n, o, taps)} input samples (o = {o}, n = {n}, taps = {taps}), above {MIX_MAX_FLOATS}')
    full = -(-n * n_in // o)
    len_out = full if len_out is None else int(len_out)
    y = torch.empty(P, len_out, device=x.device, dtype=torch.float32)
    lib = _lib.load()
    for p0 in range(0, P, per):
        pn = min(per, P - p0)
        rc = lib.sf_resample_wave_mix(xp, _MIX_DT[x.dtype], ch, x.stride(0) if ch > 1 else 1, x.stride(1) if n_in > 1 else 1, n_in, mp + 4 * ch * p0, pn, kp, n, taps,
                                      o, width, _dev(y, 'y') + 4 * len_out * p0, max(len_out, 1), len_out, _stream())
        _lib.check(rc, 'sf_resample_wave_mix')
    return y


# ----------------------------------------------------------------------------------------------------------------------
# PyTorch dispatcher registration (SURVEY §8b "custom-op contract"): the C-ABI launchers as `torch.ops.synchformer.*`
# out-variant custom ops (device_types = "cuda", i.e. HIP on ROCm).  They mutate their `out` argument and return nothing,
# which keeps them usable under torch.no_grad / autocast-free eager code and visible to the dispatcher; autograd for
# training goes through synchformer_amd.train.SyncTrainFunction, not through these leaf ops.
# ----------------------------------------------------------------------------------------------------------------------
_registered = False


# the operators libsynchformer_torch.so defines (csrc/sf_torch_library.cpp)
DISPATCHER_OPS = ('gemm_bf16', 'layernorm768', 'gemm_res_ln768', 'attention', 'attention_cls', 'attention_cls_partial', 'attention_cls_combine', 'im2col_video',
                  'qkv_time_attention', 'qkv_time_attention2', 'qkv_space_attention', 'qkv_time_attention2_masked', 'qkv_space_attention_masked', 'space_side_rows',
                  'space_side_rows_mx', 'quantize_mxfp8', 'layernorm768_mxfp8', 'gemm_mxfp8', 'gemm_mx_res_ln768', 'qkv_time_attention_mx', 'qkv_time_attention_mx_q',
                  'attention_cls_partial_mx', 'attention_cls_combine_mx', 'qkv_space_attention_mx', 'qkv_space_attention_mx_q', 'qkv_time_attention2_mx',
                  'qkv_time_attention2_mx_q')


def register_torch_ops():
    """Load the dispatcher library: `libsynchformer_torch.so` (csrc/sf_torch_library.cpp) DEFINES `torch.ops.synchformer.*` with TORCH_LIBRARY and implements
    them for the CUDA (= HIP on ROCm) dispatch key with TORCH_LIBRARY_IMPL, each operator one call into the C ABI on the current HIP stream.  Python adds what has no
    device code: the Meta / FakeTensor implementations (every op is an out-variant - it mutates its outputs and returns nothing -, so the abstract implementation only
    checks what the launcher would refuse) and the two functional ops with autograd (synchformer_amd/functional.py).  Raises if the library is not built - there is no
    Python-side fallback registration."""
    global _registered
    if _registered:
        return
    path = _lib.lib_path().parent / 'libsynchformer_torch.so'
    if not path.exists() and os.environ.get('SYNCHFORMER_HIP_LIB'):        # a measurement build given by path (tools/ab_*.sh): the dispatcher library of the package
        path = Path(__file__).resolve().parent / 'lib' / 'libsynchformer_torch.so'
    if not path.exists():
        raise RuntimeError(f'{path} not found: the dispatcher library is not built (python -c "import __graft_entry__ as g; g.build()")')
    _lib.load()                                                             # libsynchformer_hip.so first: the dispatcher library links against it
    torch.ops.load_library(str(path))

    def _fake(check=None):
        def impl(*args):
            if check is not None:
                check(*args)
            return None
        return impl

    def _chk_gemm(a, w, bias, out, residual, gelu):
        n = w.shape[1] if w.dim() == 3 else w.shape[0]
        torch._check(a.dim() == 2 and out.dim() == 2 and out.shape[0] == a.shape[0] and out.shape[1] == n, lambda: 'synchformer::gemm_bf16: out must be (M, N)')
        torch._check(a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, lambda: 'synchformer::gemm_bf16: bf16 operands')
        torch._check(out.dtype in (torch.bfloat16, torch.float32), lambda: 'synchformer::gemm_bf16: out is bf16 or fp32')

    def _chk_ln(x, gamma, beta, out, eps):
        torch._check(x.shape[-1] == 768 and out.shape[-1] == 768 and x.dtype == torch.float32, lambda: 'synchformer::layernorm768: fp32 (rows, 768) in, 768 columns out')

    torch.library.register_fake('synchformer::gemm_bf16')(_fake(_chk_gemm))
    torch.library.register_fake('synchformer::layernorm768')(_fake(_chk_ln))
    for name in DISPATCHER_OPS:
        if name not in ('gemm_bf16', 'layernorm768'):
            torch.library.register_fake('synchformer::' + name)(_fake())

    from . import functional as _functional                                 # the functional ops with autograd (synchformer::linear, ::layer_norm768)
    _functional.register()
    _registered = True


class via_dispatcher:
    """Context manager: while active, the launches the engine's default schedule is made of go through the PyTorch dispatcher
    (`torch.ops.synchformer.*`, registered above) instead of straight into the C ABI - what a torch-side integration (profiler, dispatch modes,
    `torch.library` consumers) sees.  Calls with arguments the registered schemas do not carry (row maps, explicit M) fall through to the direct path.
        with ops.via_dispatcher(): logits = engine.forward(vis, aud)
    The results are the same launches on the same buffers (tests/test_e2e_gpu.py compares them bit for bit)."""
    NAMES = ('gemm', 'layernorm', 'gemm_res_ln', 'qkv_time_attention', 'attention_cls_partial', 'attention_cls_combine', 'quantize_mxfp8', 'layernorm_mxfp8',
             'gemm_mxfp8', 'gemm_mx_res_ln', 'qkv_time_attention_mx', 'attention_cls_partial_mx', 'attention_cls_combine_mx', 'qkv_time_attention2',
             'qkv_space_attention', 'qkv_space_attention_mx', 'space_side_rows', 'space_side_rows_mx', 'qkv_time_attention2_mx')

    _depth = 0                                                    # re-entrant: an inner `with` inside an active one changes nothing
    _lock = threading.RLock()                                     # the depth counter and the module-globals swap are one critical section
    calls_total = 0                                               # launches that went through torch.ops.synchformer.* since import (all instances)

    def __init__(self):
        self.calls = 0
        self._nested = False

    def __enter__(self):
        with via_dispatcher._lock:
            if via_dispatcher._depth > 0:
                via_dispatcher._depth += 1
                self._nested = True
                return self
            register_torch_ops()                                  # raises if libsynchformer_torch.so is missing: the route is then NOT marked active (every later
            self._swap_in()                                       # `with` raises again instead of silently taking the direct path)
            via_dispatcher._depth = 1
            return self

    def _swap_in(self):
        g = globals()
        o = self.orig = {n: g[n] for n in self.NAMES}
        t = torch.ops.synchformer

        def count(fn):
            def run(*a):
                self.calls += 1
                via_dispatcher.calls_total += 1
                return fn(*a)
            return run

        def gemm_(a, w, bias, out, *, M=None, residual=None, gelu=False, c_map=None, r_map=None):
            if M is not None or c_map is not None or r_map is not None:
                return o['gemm'](a, w, bias, out, M=M, residual=residual, gelu=gelu, c_map=c_map, r_map=r_map)
            count(t.gemm_bf16)(a, w, bias, out, residual, gelu)
            return out

        def layernorm_(x, gamma, beta, out, eps, **kw):
            if kw:
                return o['layernorm'](x, gamma, beta, out, eps, **kw)
            count(t.layernorm768)(x, gamma, beta, out, eps)
            return out

        def gemm_res_ln_(a, w, bias, x, gamma, beta, y, eps, *, M=None, residual=None, period=None):
            if M is not None or residual is not None:
                return o['gemm_res_ln'](a, w, bias, x, gamma, beta, y, eps, M=M, residual=residual, period=period)
            count(t.gemm_res_ln768)(a, w, bias, x, gamma, beta, y, eps)
            return x, y

        def qkv_time_(x, w, bias, qkv_cls, out, partials, *, n_seq, n_groups, scale, key_keep=None):
            count(t.qkv_time_attention)(x, w, bias, qkv_cls, out, partials, n_seq, n_groups, scale, key_keep)
            return out

        def qkv_time_mx_(x_q, x_s, w_q, w_s, bias, qkv_cls, out, partials, *, n_seq, n_groups, scale, out_scales=None):
            if out_scales is not None:
                count(t.qkv_time_attention_mx_q)(x_q, x_s, w_q, w_s, bias, qkv_cls, out, out_scales, partials, n_seq, n_groups, scale)
                return out
            count(t.qkv_time_attention_mx)(x_q, x_s, w_q, w_s, bias, qkv_cls, out, partials, n_seq, n_groups, scale)
            return out

        def attn_part_(q, k, v, out, partials, *, n_seq, seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim, scale, key_keep=None):
            count(t.attention_cls_partial)(q, k, v, out, partials, n_seq, seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, head_dim, scale,
                                           key_keep)
            return out

        def attn_comb_(partials, out, *, n_part, n_seq, out_seq_rows, out_row, heads):
            count(t.attention_cls_combine)(partials, out, n_part, n_seq, out_seq_rows, out_row, heads)
            return out

        def quant_(x, q, scales, rows=None):
            if rows is not None:
                return o['quantize_mxfp8'](x, q, scales, rows)
            count(t.quantize_mxfp8)(x, q, scales)
            return q, scales

        def ln_mx_(x, gamma, beta, q, scales, eps, rows=None):
            if rows is not None:
                return o['layernorm_mxfp8'](x, gamma, beta, q, scales, eps, rows)
            count(t.layernorm768_mxfp8)(x, gamma, beta, q, scales, eps)
            return q, scales

        def gemm_mx_(a_q, a_s, w_q, w_s, bias, out, *, M=None, residual=None, gelu=False, out_scales=None):
            if M is not None:
                return o['gemm_mxfp8'](a_q, a_s, w_q, w_s, bias, out, M=M, residual=residual, gelu=gelu, out_scales=out_scales)
            count(t.gemm_mxfp8)(a_q, a_s, w_q, w_s, bias, out, out_scales, residual, gelu)
            return out

        def gemm_mx_ln_(a_q, a_s, w_q, w_s, bias, x, gamma, beta, y_q, y_s, eps, *, M=None, residual=None):
            if M is not None or residual is not None:
                return o['gemm_mx_res_ln'](a_q, a_s, w_q, w_s, bias, x, gamma, beta, y_q, y_s, eps, M=M, residual=residual)
            count(t.gemm_mx_res_ln768)(a_q, a_s, w_q, w_s, bias, x, gamma, beta, y_q, y_s, eps)
            return x, y_q, y_s

        def attn_part_mx_(q, k, v, out_q, out_s, partials, *, n_seq, seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, scale):
            count(t.attention_cls_partial_mx)(q, k, v, out_q, out_s, partials, n_seq, seq_rows, n_groups, row0, group_stride, tok_stride, n_tok, cls_row, heads, scale)
            return out_q

        def attn_comb_mx_(partials, out_q, out_s, *, n_part, n_seq, out_seq_rows, out_row, heads):
            count(t.attention_cls_combine_mx)(partials, out_q, out_s, n_part, n_seq, out_seq_rows, out_row, heads)
            return out_q

        def qkv_time2_(x, w, bias, side, out, partials, *, n_seq, scale, n_tok=196, key_keep=None):
            if key_keep is not None:
                count(t.qkv_time_attention2_masked)(x, w, bias, side, out, partials, n_seq, scale, key_keep)
                return out
            count(t.qkv_time_attention2)(x, w, bias, side, out, partials, n_seq, scale)
            return out

        def qkv_space_(x, w, bias, side, out, partials, *, n_seq, scale, n_tok=196, key_keep=None):
            if key_keep is not None:
                count(t.qkv_space_attention_masked)(x, w, bias, side, out, partials, n_seq, scale, key_keep)
                return out
            count(t.qkv_space_attention)(x, w, bias, side, out, partials, n_seq, scale)
            return out

        def qkv_space_mx_(x_q, x_s, w_q, w_s, bias, side, out, partials, *, n_seq, scale, out_scales=None, n_tok=196):
            if out_scales is not None:
                count(t.qkv_space_attention_mx_q)(x_q, x_s, w_q, w_s, bias, side, out, out_scales, partials, n_seq, scale)
                return out
            count(t.qkv_space_attention_mx)(x_q, x_s, w_q, w_s, bias, side, out, partials, n_seq, scale)
            return out

        def side_rows_(x, out, n_seq):
            count(t.space_side_rows)(x, out, n_seq)
            return out

        def side_rows_mx_(x_q, x_s, side_q, side_s, n_seq):
            count(t.space_side_rows_mx)(x_q, x_s, side_q, side_s, n_seq)
            return side_q, side_s

        def qkv_time2_mx_(x_q, x_s, w_q, w_s, bias, side, out, partials, *, n_seq, scale, out_scales=None, n_tok=196):
            if out_scales is not None:
                count(t.qkv_time_attention2_mx_q)(x_q, x_s, w_q, w_s, bias, side, out, out_scales, partials, n_seq, scale)
                return out
            count(t.qkv_time_attention2_mx)(x_q, x_s, w_q, w_s, bias, side, out, partials, n_seq, scale)
            return out

        g.update(attention_cls_partial_mx=attn_part_mx_, attention_cls_combine_mx=attn_comb_mx_, qkv_time_attention2=qkv_time2_, qkv_space_attention=qkv_space_,
                 qkv_space_attention_mx=qkv_space_mx_, space_side_rows=side_rows_, space_side_rows_mx=side_rows_mx_, qkv_time_attention2_mx=qkv_time2_mx_)
        g.update(gemm=gemm_, layernorm=layernorm_, gemm_res_ln=gemm_res_ln_, qkv_time_attention=qkv_time_, attention_cls_partial=attn_part_,
                 attention_cls_combine=attn_comb_, quantize_mxfp8=quant_, layernorm_mxfp8=ln_mx_, gemm_mxfp8=gemm_mx_, gemm_mx_res_ln=gemm_mx_ln_,
                 qkv_time_attention_mx=qkv_time_mx_)

    def __exit__(self, *exc):
        with via_dispatcher._lock:
            via_dispatcher._depth -= 1
            if self._nested:
                self._nested = False
                return
            globals().update(self.orig)
