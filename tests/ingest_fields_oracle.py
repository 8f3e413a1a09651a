"""Oracle of the interlaced ingest, shared by test_ingest_fields_cpu.py, test_ingest_fields_gpu.py and tests/golden/make_ingest_fields_digests.py.  It does
not import synchformer_amd.ingest: a field is sliced out of its frame with plain indexing (rows p, p + 2, ..), every plane of it is resized with
ingest_yuv16_oracle.resize_dense to the FRAME's (Hr, Wr) with the vertical shift +0.25 (parity 0) or -0.25 (parity 1) - frame row 2 k + p has its centre at frame
coordinate 2 k + p + 0.5, which is field coordinate k + 0.5 + 0.25 - p / 2 - and the pick, the packings, the matrices and the pixel bar are the existing oracles'."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_oracle import check_pixels, frame_table_bruteforce, random_frames  # noqa: E402,F401
from ingest_yuv_oracle import apply_tables32, origin  # noqa: E402,F401
from ingest_yuv16_oracle import dense_filter, resize_dense  # noqa: E402,F401
from ingest_yuv422_oracle import FMTS, FMTS_16, LOCS, matrix, pack, random_planes  # noqa: E402,F401

CROP = 224
ORDERS = ('tff', 'bff')
TABLE = [0, 1, 1, 4, 7]                                                          # the FIELD pick of the GPU tests over 4 frames: both parities, a repeat and a skip
SHIFT_Y = (0.25, -0.25)                                                          # vertical shift of the filter centre for the field of parity 0 / 1, in field rows
# (H, W) -> (colorspace, full_range, chroma_loc, field taps (y, x), chroma taps (y, x)): landscape (field 135 rows); portrait (the field is upscaled vertically, chroma
# width 101); 1080i (wide-row chunks, the 11-tap field filter)
CASES = {(270, 480): ('bt601', False, 'left', (5, 7), (5, 5)), (480, 202): ('bt709', True, 'center', (5, 5), (5, 5)),
         (1080, 1920): ('bt709', False, 'left', (11, 19), (11, 11))}


def parity(f: int, order: str) -> int:
    """The rows of temporal field f: p = f & 1 top field first, the other one bottom field first."""
    assert order in ORDERS
    return (f & 1) ^ (order == 'bff')


def field(x: torch.Tensor, f: int, order: str) -> torch.Tensor:
    """Field f of frames x (n, ..., H, W): rows p, p + 2, .. of frame f >> 1."""
    return x[f >> 1][..., parity(f, order)::2, :]


def resize_field(x: torch.Tensor, p: int, size, y0: int, x0: int, shift_x: float = 0.0) -> torch.Tensor:
    """One field's plane(s) (..., H / 2, W) of parity p -> float64 (..., 224, 224): the frame's target size, then the frame's crop."""
    return resize_dense(x, size, SHIFT_Y[p], shift_x)[..., y0:y0 + CROP, x0:x0 + CROP]


def oracle_rgb(frames: torch.Tensor, order: str, table, size, y0: int, x0: int) -> torch.Tensor:
    """frames uint8 (n, 3, H, W) -> uint8 (len(table), 3, 224, 224): output j is field table[j], resized on its own, rounded once (half to even)."""
    done = {f: resize_field(field(frames, f, order), parity(f, order), size, y0, x0).round().clamp(0, 255).to(torch.uint8) for f in sorted(set(table))}
    return torch.stack([done[f] for f in table])


def oracle_yuv(planes, order: str, table, size, y0: int, x0: int, M: torch.Tensor, off: torch.Tensor, loc: str = 'center'):
    """4:2:2 planes Y (n, H, W), U and V (n, H, W / 2) -> (uint8 (len(table), 3, 224, 224), share outside [0, 255] before the clamp): every plane of field table[j]
    through the same vertical filter (full vertical chroma resolution), chroma shifted horizontally by LOCS[loc], rgb = M (yuv - off) in float64."""
    pre = {}
    for f in sorted(set(table)):
        p = parity(f, order)
        r = [resize_field(field(pl, f, order), p, size, y0, x0, 0.0 if k == 0 else LOCS[loc]) for k, pl in enumerate(planes)]
        pre[f] = torch.einsum('ck,kyx->cyx', M, torch.stack([r[0] - off[0], r[1] - off[1], r[2] - off[2]]))
    pre = torch.stack([pre[f] for f in table])
    return pre.round().clamp(0, 255).to(torch.uint8), ((pre < 0) | (pre > 255)).double().mean().item()


def still(H: int, W: int) -> torch.Tensor:
    """The still picture of the siting tests: round(128 + 100 sin(2 pi 3 (y + 1/2) / H) cos(2 pi (x + 1/2) / W)), uint8 (H, W)."""
    y = (torch.arange(H, dtype=torch.float64) + 0.5) / H
    x = (torch.arange(W, dtype=torch.float64) + 0.5) / W
    return (128 + 100 * torch.sin(2 * torch.pi * 3 * y)[:, None] * torch.cos(2 * torch.pi * x)[None]).round().to(torch.uint8)


def rgb_frames(H: int, W: int) -> torch.Tensor:
    """The 4 source frames of the rgb24 GPU cases and digests: uint8 (4, 3, H, W)."""
    return random_frames(4, H, W, H * 10000 + W)


def yuv_planes(H: int, W: int, bits: int):
    """The 4 source frames of the 4:2:2 GPU cases and digests as planes: Y (4, H, W), U and V (4, H, W / 2), int32 samples of `bits` bits."""
    return random_planes(4, H, W, H * 10000 + W + bits, 1 << bits)
