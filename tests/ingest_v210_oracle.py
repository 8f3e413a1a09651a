"""Oracle of the v210 ingest, shared by test_ingest_v210_cpu.py and test_ingest_v210_gpu.py.  It does not import synchformer_amd.ingest.  The packing
is written from the format's definition - a row of W pixels is the 10-bit fields Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 .., field F in little-endian 32-bit word F // 3 at bit
10 (F % 3), bits 30 - 31 unused, whole groups of four words per six pixels - as index arithmetic over the field number F; the resize, the matrices and the pixel bar
are ingest_yuv422_oracle's (float64 dense filters, one rounding), imported, on the planes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_yuv422_oracle import CASES as CASES_422, LOCS, TABLE, check_pixels, matrix, oracle, origin, pack, random_planes  # noqa: E402,F401

# (H, W) -> (colorspace, full_range, chroma_loc, luma taps (y, x), chroma taps (y, x)): the four cases of the 4:2:2 oracle, and two widths for the group arithmetic -
# (540, 958): W % 12 == 10, the landscape crop origin off the 12-column grid; (480, 202): portrait, the row is upscaled, W % 6 == 4, chroma width 101
CASES = dict(CASES_422)
CASES[(540, 958)] = ('bt709', True, 'left', (11, 11), (11, 7))
CASES[(480, 202)] = ('bt601', False, 'center', (5, 5), (5, 5))


def min_words(W: int) -> int:
    """Words of a row of W pixels: four per group of six pixels, whole groups."""
    return 4 * -(-W // 6)


def field_planes(planes) -> np.ndarray:
    """Planes Y (n, H, W), U and V (n, H, W / 2) -> the fields of every row in stream order, int64 (n, H, 2 W): field 4 j = Cb[j], 4 j + 2 = Cr[j], 2 x + 1 = Y[x]."""
    Y, U, V = (np.asarray(p, dtype=np.int64) for p in planes)
    n, H, W = Y.shape
    assert W % 2 == 0 and U.shape == V.shape == (n, H, W // 2)
    f = np.zeros((n, H, 2 * W), dtype=np.int64)
    f[..., 0::4] = U
    f[..., 2::4] = V
    f[..., 1::2] = Y
    return f


def pack_v210(planes, row_words=None, fill: int = 0) -> torch.Tensor:
    """Planes of 10-bit samples -> v210 frames int32 (n, H, row_words) (the bits of the uint32 words).  row_words: None = the minimal 4 ceil(W / 6).  fill: the 32-bit
    value of every padding word, whose 10-bit fields also fill the unused trailing fields of a last partial group; bits 30 - 31 of the words that hold samples are 0."""
    f = field_planes(planes)
    n, H, nf = f.shape
    W = nf // 2
    need = min_words(W)
    row_words = need if row_words is None else int(row_words)
    assert row_words >= need and 0 <= fill <= 0xffffffff and int(f.min()) >= 0 and int(f.max()) <= 1023
    words = np.full((n, H, row_words), fill, dtype=np.uint64)
    F = np.arange(nf)
    for pos in range(3):                                                        # the fields at bit 10 pos of their word
        sel = F[F % 3 == pos]
        w = sel // 3
        words[..., w] = (words[..., w] & np.uint64(0xffffffff ^ (1023 << (10 * pos)))) | (f[..., sel].astype(np.uint64) << np.uint64(10 * pos))
    last = (nf - 1) // 3                                                        # the word of the last field: the words that hold samples keep bits 30 - 31 clear
    words[..., :last + 1] &= np.uint64(0x3fffffff)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32).copy())


def unpack_v210(raw: torch.Tensor, W: int):
    """v210 frames int32 / uint32 (n, H, Pw) -> planes Y (n, H, W), U and V (n, H, W / 2), int32."""
    words = raw.contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.int64)
    F = np.arange(2 * W)
    f = (words[..., F // 3] >> (10 * (F % 3))) & 1023
    return [torch.from_numpy(np.ascontiguousarray(p)).to(torch.int32) for p in (f[..., 1::2], f[..., 0::4], f[..., 2::4])]


def set_stray_bits(raw: torch.Tensor) -> torch.Tensor:
    """The same frames with bits 30 - 31 set in every word."""
    return torch.from_numpy((raw.contiguous().numpy().view(np.uint32) | np.uint32(0xc0000000)).view(np.int32).copy())
