"""Oracle of the YUV 4:2:0 ingest, shared by test_ingest_yuv_cpu.py and test_ingest_yuv_gpu.py.  It does not call synchformer_amd.ingest: the
resize is ingest_oracle.resize64 (torch's own CPU F.interpolate on float64) of each plane, chroma as an (H / 2, W / 2) image, the crop origin is RGBSpatialCrop's,
and the colour matrix is written out here from Kr, Kb, the range gains and the offsets - float64 end to end, one rounding at the end."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_oracle import TABLE, check_pixels, resize64  # noqa: E402,F401  (the frame pick and the pixel bar are shared with test_ingest_gpu.py)

CROP = 224
# (H, W) -> (colorspace, full_range, luma taps (y, x), chroma taps (y, x))
CASES = {(270, 480): ('bt601', False, (7, 7), (5, 5)), (360, 202): ('bt709', True, (5, 5), (5, 5)), (144, 176): ('bt601', False, (5, 5), (5, 5)),
         (540, 960): ('bt709', True, (11, 11), (7, 7)), (302, 518): ('bt601', False, (7, 7), (5, 5)), (1080, 608): ('bt709', True, (11, 11), (7, 7))}


def matrix64(colorspace: str, full_range: bool):
    """(M (3, 3), offsets (3,)) float64: rgb = M @ (yuv - offsets)."""
    kr, kb = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}[colorspace]
    kg = 1.0 - kr - kb
    gy, gc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    cr, cb = 2.0 * (1.0 - kr) * gc, 2.0 * (1.0 - kb) * gc                        # R from V', B from U'
    M = torch.tensor([[gy, 0.0, cr], [gy, -cb * kb / kg, -cr * kr / kg], [gy, cb, 0.0]], dtype=torch.float64)
    return M, torch.tensor([0.0 if full_range else 16.0, 128.0, 128.0], dtype=torch.float64)


def origin(H: int, W: int, side: int = 256):
    """(Hr, Wr, y0, x0): the short side to `side`, the other one cut to even, the centre crop's origin."""
    Hr, Wr = (side, (W * side // H) // 2 * 2) if H <= W else ((H * side // W) // 2 * 2, side)
    return Hr, Wr, int(round((Hr - CROP) / 2.)), int(round((Wr - CROP) / 2.))


def random_planes(n: int, H: int, W: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8) for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]


def pack(Y: torch.Tensor, U: torch.Tensor, V: torch.Tensor, pix_fmt: str) -> torch.Tensor:
    """Planes (n, H, W), (n, H / 2, W / 2) x 2 -> uint8 (n, 3 H / 2, W): 'nv12' (H luma rows, H / 2 rows of interleaved U V) or 'yuv420p' (I420: the luma
    bytes, the U plane, the V plane, back to back)."""
    n, H, W = Y.shape
    if pix_fmt == 'nv12':
        return torch.cat([Y, torch.stack([U, V], -1).reshape(n, H // 2, W)], 1).contiguous()
    assert pix_fmt == 'yuv420p'
    return torch.cat([Y.reshape(n, -1), U.reshape(n, -1), V.reshape(n, -1)], 1).reshape(n, H * 3 // 2, W).contiguous()


def convert64(Yr, Ur, Vr, colorspace: str, full_range: bool) -> torch.Tensor:
    """Resized float64 planes (n, h, w) -> RGB float64 (n, 3, h, w) before rounding."""
    M, off = matrix64(colorspace, full_range)
    return torch.einsum('ck,nkyx->ncyx', M, torch.stack([Yr - off[0], Ur - off[1], Vr - off[2]], 1))


def oracle(planes, size, y0: int, x0: int, colorspace: str, full_range: bool):
    """uint8 (n, 3, 224, 224) and the share of values that were outside [0, 255] before the clamp."""
    r = [resize64(p, size)[..., y0:y0 + CROP, x0:x0 + CROP] for p in planes]
    pre = convert64(*r, colorspace, full_range)
    return pre.round().clamp(0, 255).to(torch.uint8), ((pre < 0) | (pre > 255)).double().mean().item()


def apply_tables32(plane: torch.Tensor, yf, yw, xf, xw) -> torch.Tensor:
    """The kernel's arithmetic restated in fp32 on the CPU: plane (n, h, w) uint8, tables sliced to the crop (first (224,), weights (224, taps)); horizontal pass
    first, taps in ascending order, zero-weight taps past the edge read zeros."""
    x = torch.nn.functional.pad(plane.float(), (0, xw.shape[1], 0, yw.shape[1]))
    h = torch.zeros(*x.shape[:2], CROP)
    for k in range(xw.shape[1]):
        h = h + xw[:, k] * x[:, :, xf.long() + k]
    out = torch.zeros(x.shape[0], CROP, CROP)
    for i in range(yw.shape[1]):
        out = out + yw[:, i, None] * h[:, yf.long() + i]
    return out

