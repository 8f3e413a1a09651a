"""Oracle of the 4:2:2 ingest, shared by test_ingest_yuv422_cpu.py and test_ingest_yuv422_gpu.py.  It does not import synchformer_amd.ingest: the
resize is the dense float64 filter matrix per axis of ingest_yuv16_oracle (written out from the filter's formula with the centre c = scale (i + 0.5) + shift), the
chroma planes are (H, W / 2) images - no vertical subsampling, so only a horizontal siting shift exists - the colour matrices are ingest_yuv_oracle.matrix64 and
its 10-bit counterpart, the seven layouts are packed here from their published byte orders, and everything is float64 with one rounding at the end."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_oracle import TABLE, check_pixels  # noqa: E402,F401  (the frame pick and the pixel bar are the project's own, unchanged)
from ingest_yuv_oracle import apply_tables32, matrix64, origin  # noqa: E402,F401
from ingest_yuv16_oracle import dense_filter, matrix64_10, resize_dense  # noqa: E402,F401

CROP = 224
FMTS = ('uyvy422', 'yuyv422', 'yuv422p', 'nv16', 'yuv422p10le', 'p210', 'y210')
FMTS_16 = ('yuv422p10le', 'p210', 'y210')
SHIFT = {'yuv422p10le': 0, 'p210': 6, 'y210': 6}
LOCS = {'center': 0.0, 'left': 0.25, 'topleft': 0.25}                            # horizontal shift of the chroma filter centre, in chroma samples; never a vertical one
# (H, W) -> (colorspace, full_range, chroma_loc, luma taps (y, x), chroma taps (y, x))
CASES = {(270, 480): ('bt601', False, 'left', (7, 7), (7, 5)), (271, 202): ('bt709', True, 'center', (5, 5), (5, 5)),
         (144, 176): ('bt601', False, 'left', (5, 5), (5, 5)), (540, 960): ('bt709', True, 'left', (11, 11), (11, 7))}


def random_planes(n: int, H: int, W: int, seed: int, levels: int = 256):
    """Uniform random samples in [0, levels), int32: Y (n, H, W), U and V (n, H, W / 2)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, levels, (n, h, w), generator=g, dtype=torch.int32) for h, w in ((H, W), (H, W // 2), (H, W // 2))]


def pack(planes, pix_fmt: str) -> torch.Tensor:
    """Planes Y (n, H, W), U and V (n, H, W / 2), int32 sample values (8-bit, or 10-bit for FMTS_16) -> the raw frames of the format:
    uyvy422 / yuyv422  uint8  (n, H, W, 2)   bytes U0 Y0 V0 Y1 / Y0 U0 Y1 V0 per two columns
    y210               uint16 (n, H, W, 2)   words Y0 U0 Y1 V0, the sample in the HIGH ten bits
    nv16 / p210        uint8 / uint16 (n, 2 H, W)   H luma rows, then H rows of interleaved U V (p210: the sample in the high ten bits)
    yuv422p / yuv422p10le   uint8 / uint16 (n, 2 H, W)   the luma samples, the U plane, the V plane, back to back (10le: the sample in the low ten bits)."""
    Y, U, V = planes
    n, H, W = Y.shape
    assert U.shape == V.shape == (n, H, W // 2) and W % 2 == 0 and pix_fmt in FMTS
    dtype = torch.uint16 if pix_fmt in FMTS_16 else torch.uint8
    sh = SHIFT.get(pix_fmt, 0)
    Ye = Y.reshape(n, H, W // 2, 2)
    if pix_fmt == 'uyvy422':
        raw = torch.stack([U, Ye[..., 0], V, Ye[..., 1]], -1).reshape(n, H, W, 2)
    elif pix_fmt in ('yuyv422', 'y210'):
        raw = torch.stack([Ye[..., 0], U, Ye[..., 1], V], -1).reshape(n, H, W, 2)
    elif pix_fmt in ('nv16', 'p210'):
        raw = torch.cat([Y, torch.stack([U, V], -1).reshape(n, H, W)], 1)
    else:
        raw = torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], 1).reshape(n, 2 * H, W)
    return (raw << sh).to(dtype).contiguous()


def oracle(planes, size, y0: int, x0: int, M: torch.Tensor, off: torch.Tensor, loc: str = 'center', shift_y: float = 0.0):
    """uint8 (n, 3, 224, 224) and the share of values outside [0, 255] before the clamp: luma through the unshifted filter, chroma - planes of any size - through
    the filter shifted horizontally by LOCS[loc] (and vertically by shift_y: 0 for 4:2:2), cropped, rgb = M (yuv - off) in float64, rounded once (half to even)."""
    r = [resize_dense(p, size, *((0.0, 0.0) if k == 0 else (shift_y, LOCS[loc])))[..., y0:y0 + CROP, x0:x0 + CROP] for k, p in enumerate(planes)]
    pre = torch.einsum('ck,nkyx->ncyx', M, torch.stack([r[0] - off[0], r[1] - off[1], r[2] - off[2]], 1))
    return pre.round().clamp(0, 255).to(torch.uint8), ((pre < 0) | (pre > 255)).double().mean().item()


def matrix(colorspace: str, full_range: bool, bits: int):
    """(M, offsets) float64 on the 8-bit or the 10-bit sample scale."""
    return matrix64(colorspace, full_range) if bits == 8 else matrix64_10(colorspace, full_range)
