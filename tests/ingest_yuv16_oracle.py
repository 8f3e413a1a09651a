"""Oracle of the 10-bit YUV 4:2:0 ingest and of sited chroma, shared by test_ingest_yuv16_cpu.py and test_ingest_yuv16_gpu.py.  It does not import
synchformer_amd.ingest: the resize is a dense float64 matrix per axis written out here from the filter's formula with the centre c = scale (i + 0.5) + shift
(pinned by the CPU test: at shift 0 it is ingest_oracle.resize64, torch's own F.interpolate on float64, to 1e-9), the 10-bit colour matrix is written out here
from Kr, Kb, the range gains and the offsets, and everything is float64 with one rounding at the end."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_oracle import TABLE, check_pixels, resize64  # noqa: E402,F401  (the frame pick and the pixel bar are the project's own, unchanged)
from ingest_yuv_oracle import apply_tables32, matrix64, origin  # noqa: E402,F401  (the fp32 restatement of the kernel's arithmetic, the 8-bit matrix, the crop origin)

CROP = 224
FMTS = ('p010', 'yuv420p10le')
SHIFT = {'p010': 6, 'yuv420p10le': 0}
LOCS = {'center': (0.0, 0.0), 'left': (0.0, 0.25), 'topleft': (0.25, 0.25)}          # (vertical, horizontal) shift of the chroma filter centre, in chroma samples
# (H, W) -> (colorspace, full_range, chroma_loc): the four settings of the pixel bar, and (360, 202) for the unaligned chroma rows (chroma width 101)
CASES = {(270, 480): ('bt709', False, 'left'), (1080, 608): ('bt601', True, 'center'), (144, 176): ('bt709', False, 'left'), (540, 960): ('bt601', False, 'left'),
         (360, 202): ('bt601', False, 'topleft')}


def dense_filter(n_in: int, n_out: int, shift: float = 0.0) -> torch.Tensor:
    """(n_out, n_in) float64: row i holds the antialiased bicubic filter (a = -0.5) centred at c = scale (i + 0.5) + shift, source sample j at coordinate j + 0.5,
    stretched by scale when downscaling, cut to the source samples [int(c - support + 0.5), int(c + support + 0.5)) inside the picture, normalised to sum 1."""
    scale = n_in / n_out
    stretch = max(scale, 1.0)
    support = 2.0 * stretch
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5) + shift
        lo, hi = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        row = []
        for j in range(lo, hi):
            t = abs((j + 0.5 - c) / stretch)
            row.append(1.5 * t ** 3 - 2.5 * t ** 2 + 1.0 if t < 1 else -0.5 * t ** 3 + 2.5 * t ** 2 - 4.0 * t + 2.0 if t < 2 else 0.0)
        A[i, lo:hi] = torch.tensor(row, dtype=torch.float64) / math.fsum(row)
    return A


def resize_dense(x: torch.Tensor, size, shift_y: float = 0.0, shift_x: float = 0.0) -> torch.Tensor:
    """x (..., h, w) any dtype -> float64 (..., Hr, Wr) = Ay x Ax^T."""
    return dense_filter(x.shape[-2], size[0], shift_y) @ x.double() @ dense_filter(x.shape[-1], size[1], shift_x).T


def matrix64_10(colorspace: str, full_range: bool):
    """(M (3, 3), offsets (3,)) float64 with rgb8 = M @ (yuv10 - offsets): limited range maps luma [64, 940] and chroma [64, 960] (219 * 4 and 224 * 4 steps) to
    [0, 255], full range maps [0, 1023]."""
    kr, kb = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}[colorspace]
    kg = 1.0 - kr - kb
    gy, gc = (255.0 / 1023.0, 255.0 / 1023.0) if full_range else (255.0 / 876.0, 255.0 / 896.0)
    cr, cb = 2.0 * (1.0 - kr) * gc, 2.0 * (1.0 - kb) * gc
    M = torch.tensor([[gy, 0.0, cr], [gy, -cb * kb / kg, -cr * kr / kg], [gy, cb, 0.0]], dtype=torch.float64)
    return M, torch.tensor([0.0 if full_range else 64.0, 512.0, 512.0], dtype=torch.float64)


def random_planes(n: int, H: int, W: int, seed: int, levels: int = 1024):
    """Uniform random samples in [0, levels), int32: Y (n, H, W), U and V (n, H / 2, W / 2)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, levels, (n, h, w), generator=g, dtype=torch.int32) for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]


def pack(Y: torch.Tensor, U: torch.Tensor, V: torch.Tensor, pix_fmt: str) -> torch.Tensor:
    """10-bit planes (int32) -> uint16 (n, 3 H / 2, W): 'p010' (H luma rows, H / 2 rows of interleaved U V, the sample in the HIGH ten bits) or 'yuv420p10le'
    (the luma samples, the U plane, the V plane, back to back, the sample in the LOW ten bits)."""
    n, H, W = Y.shape
    if pix_fmt == 'p010':
        return (torch.cat([Y, torch.stack([U, V], -1).reshape(n, H // 2, W)], 1) << 6).to(torch.uint16).contiguous()
    assert pix_fmt == 'yuv420p10le'
    return torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], 1).reshape(n, H * 3 // 2, W).to(torch.uint16).contiguous()


def oracle(planes, size, y0: int, x0: int, M: torch.Tensor, off: torch.Tensor, loc: str = 'center'):
    """uint8 (n, 3, 224, 224) and the share of values outside [0, 255] before the clamp: luma through the unshifted filter, chroma through the filter shifted by
    LOCS[loc], cropped, rgb = M (yuv - off) in float64, rounded once (half to even)."""
    sy, sx = LOCS[loc]
    r = [resize_dense(p, size, *((0.0, 0.0) if k == 0 else (sy, sx)))[..., y0:y0 + CROP, x0:x0 + CROP] for k, p in enumerate(planes)]
    pre = torch.einsum('ck,nkyx->ncyx', M, torch.stack([r[0] - off[0], r[1] - off[1], r[2] - off[2]], 1))
    return pre.round().clamp(0, 255).to(torch.uint8), ((pre < 0) | (pre > 255)).double().mean().item()
