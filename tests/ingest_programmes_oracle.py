"""Oracle of sf_resample_wave_mix, shared by test_ingest_programmes_cpu.py and test_ingest_programmes_gpu.py: the mix and the polyphase bank written
from the definition in float64, numpy only.  It calls neither synchformer_amd.ops nor synchformer_amd.ingest:

    xf[c, s]   = x[c, s] * scale                      scale: 1 (fp32), 2^-15 (int16), 2^-31 (int32)
    m_p[s]     = sum_c mix[p, c] xf[c, s]             0 outside [0, len)
    y[p, q n + r] = sum_i mpad_p[q o + i] kernel[r, i],   mpad_p[m] = m_p[m - width],   i < 2 width + o,   cut to ceil(n len / o)

with kernel the windowed-sinc bank of torchaudio.functional.resample at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) and, at equal rates,
the identity bank (1 x 1, width 0) RecordingIngest sends through the kernel."""
import math

import numpy as np

SCALE = {np.dtype(np.float32): 1.0, np.dtype(np.int16): 2.0 ** -15, np.dtype(np.int32): 2.0 ** -31}


def bank64(rate_in: int, rate_out: int = 16000, lpw: int = 6, rolloff: float = 0.99):
    """(kernel float64 (n, 2 width + o), width, o, n)."""
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    if o == n == 1:
        return np.ones((1, 1)), 0, 1, 1
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    k = np.empty((n, 2 * width + o))
    for r in range(n):
        for i in range(2 * width + o):
            t = min(max((-r / n + (i - width) / o) * base, -lpw), lpw)
            win = math.cos(t * math.pi / lpw / 2) ** 2
            k[r, i] = (1.0 if t == 0 else math.sin(t * math.pi) / (t * math.pi)) * win * (base / o)
    return k, width, o, n


def span(rate_in: int, rate_out: int = 16000, tile: int = 256) -> int:
    """Input samples one tile of `tile` outputs may span: ((tile - 1) // n + 1) o + taps."""
    k, width, o, n = bank64(rate_in, rate_out)
    return ((tile - 1) // n + 1) * o + k.shape[1]


def mix_resample64(x: np.ndarray, mix: np.ndarray, rate_in: int, rate_out: int = 16000) -> np.ndarray:
    """x (ch, len) float32 / int16 / int32, mix (P, ch) -> float64 (P, ceil(n len / o))."""
    k, width, o, n = bank64(rate_in, rate_out)
    xf = x.astype(np.float64) * SCALE[x.dtype]
    m = mix.astype(np.float64) @ xf                                              # (P, len)
    length = x.shape[1]
    len_out = -(-n * length // o)
    nq = -(-len_out // n) if len_out else 0
    mp = np.zeros((mix.shape[0], width + max(length, nq * o) + width + o))
    mp[:, width:width + length] = m
    y = np.zeros((mix.shape[0], nq * n))
    for q in range(nq):
        y[:, q * n:(q + 1) * n] = mp[:, q * o:q * o + k.shape[1]] @ k.T
    return y[:, :len_out]
