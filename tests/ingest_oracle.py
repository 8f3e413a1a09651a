"""Oracles of the ingest stage, shared by test_ingest_cpu.py and test_ingest_gpu.py.  None of them calls synchformer_amd.ingest:
the frame pick is a brute-force restatement of the fps filter's "near" rule, the resize is torch's own CPU F.interpolate on float64, and the resampler is
torchaudio.functional.resample's algorithm (sinc_interp_hann, its defaults) restated in float64 with F.conv1d - torchaudio itself is not a dependency."""
import math
from fractions import Fraction

import torch
import torch.nn.functional as F

SIZES = [(270, 480), (360, 202), (144, 176), (540, 960), (301, 517), (256, 256)]
TABLE = [0, 0, 2, 4, 4]                                                          # the frame pick of the GPU tests: a repeat and a skip


def frame_table_bruteforce(n_in, fps_in: Fraction, fps_out: Fraction = Fraction(25)):
    """p_i = floor(i fps_out / fps_in + 1/2);  T_out = p_{n_in - 1} + 1;  src[j] = max{i : p_i <= j}, every j searched over every i."""
    p = [(2 * i * fps_out.numerator * fps_in.denominator + fps_out.denominator * fps_in.numerator) // (2 * fps_out.denominator * fps_in.numerator) for i in range(n_in)]
    return [max(i for i in range(n_in) if p[i] <= j) for j in range(p[-1] + 1)]


def resize64(x: torch.Tensor, size) -> torch.Tensor:
    """x (..., H, W) any dtype -> float64 (..., Hr, Wr): F.interpolate(mode='bicubic', antialias=True, align_corners=False) on float64, CPU."""
    x = x.double()
    lead = x.shape[:-2]
    y = F.interpolate(x.reshape(-1, 1, *x.shape[-2:]), size=tuple(size), mode='bicubic', antialias=True, align_corners=False)
    return y.reshape(*lead, *size)


def random_frames(n: int, H: int, W: int, seed: int) -> torch.Tensor:
    """Uniform random bytes, planar uint8 (n, 3, H, W), from a CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)


def check_pixels(got: torch.Tensor, ref: torch.Tensor, what: str):
    """Every pixel within 1 level of the float64 oracle; pixels that differ at all are at most 1e-3 of all pixels (a pixel differs when fp32 and float64 land on
    opposite sides of a rounding boundary; the fp32 evaluation of the same tables on the CPU does so on <= 2e-5 of the pixels at these sizes)."""
    assert got.dtype == torch.uint8 and got.shape == ref.shape, (got.dtype, got.shape)
    d = (got.cpu().int() - ref.int()).abs()
    share = (d != 0).float().mean().item()
    print(f'{what}: max |level difference| {int(d.max())}, share of differing pixels {share:.2e}')
    assert int(d.max()) <= 1, int(d.max())
    assert share <= 1e-3, share


def resample64(x: torch.Tensor, rate_in: int, rate_out: int = 16000, lpw: int = 6, rolloff: float = 0.99, dtype=torch.float64) -> torch.Tensor:
    """x (n,) -> (ceil(rate_out n / rate_in),) in `dtype`: the polyphase windowed-sinc resampler, kernel and convolution in `dtype`."""
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
    t = (t * base).clamp(-lpw, lpw)
    win = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * win * (base / o)          # (n, 1, 2 width + o)
    xp = F.pad(x.to(dtype)[None, None], (width, width + o))
    y = F.conv1d(xp, k.to(dtype), stride=o)                                      # (1, n, q)
    y = y.transpose(1, 2).reshape(-1)
    return y[:-(-n * x.numel() // o)]
