"""Ingest a decoded recording at its native frame rate, size, pixel format and sample rate.

The reference re-encodes every input through an ffmpeg subprocess before any of its code runs (example.py:16-53: fps=25, short side scaled to 256, dimensions
cropped to even, -ar 16000) and then takes the centre 224 crop of RGBSpatialCrop.  Here the same step is host geometry (this module: pure Python / torch,
no device needed) plus two launches (ops.ingest_video: frame pick + antialiased bicubic resize + crop; ops.resample_wave: zero-delay polyphase resampler):

    ing = RecordingIngest(dev, fps_in=(30000, 1001), size_in=(1080, 1920), rate_in=48000, channels_last=True)
    track = tracker.track_raw(raw_frames, raw_wave, ing)        # raw_frames (T, 1080, 1920, 3) uint8, raw_wave (2, n) int16 or fp32; device or host

What is pinned: the frame pick restates the documented "near" rounding of ffmpeg's fps filter; the resize is F.interpolate(mode='bicubic', antialias=True,
align_corners=False) (NOT swscale's bicubic: no bit parity with an ffmpeg build is claimed or checkable here); the resampler is
torchaudio.functional.resample at its defaults (sinc_interp_hann), not swresample.

Frames may also arrive as the 8-bit YUV 4:2:0 a decoder produces, half the bytes of RGB:

    ing = RecordingIngest(dev, (30000, 1001), (1080, 1920), 48000, pix_fmt='nv12')      # or 'yuv420p': PyAV's frame.to_ndarray(format='yuv420p')
    track = tracker.track_raw(raw_frames, raw_wave, ing)        # raw_frames (T, 1620, 1920) uint8: H luma rows, then the chroma rows

The planes are resized and the colour matrix (csc_matrix: bt601 or bt709, limited or full range) runs on the 224 x 224 result, in the reference's order (its
ffmpeg step scales in YUV).  The default, bt601 limited range, is what swscale assumes for an untagged stream - an assumption that cannot be checked without an
ffmpeg build.

10-bit 4:2:0 (HEVC Main10, AV1, VP9 profile 2) arrives as uint16 (T, 3 H / 2, W) and takes the same path on 16-bit samples (ops.ingest_video_yuv16):

    ing = RecordingIngest(dev, 25, (2160, 3840), 48000, pix_fmt='p010', colorspace='bt709', chroma_loc='left')     # or 'yuv420p10le' (libav / PyAV arrays)

chroma_loc says where the chroma samples sit: 'center' (the default: chroma as an (H / 2, W / 2) image), 'left' (co-sited with the even luma columns: the default
of H.264, HEVC and MPEG-2) or 'topleft' (the BT.2020 default) - a quarter of a chroma sample in the chroma tables (aa_bicubic_table(shift=0.25)), for every YUV
format.  csc=(M, offsets) overrides colorspace / full_range with a matrix on the format's own sample scale: this is how BT.2020 coefficients are passed.

4:2:2 is what a live feed delivers - capture cards hand out packed 'uyvy422' / 'yuyv422', contribution codecs decode to 'yuv422p' / 'yuv422p10le',
hardware surfaces are 'nv16' / 'p210' / 'y210' - and goes through the general entry (ops.ingest_video_planes over plane_layout):

    ing = RecordingIngest(dev, 50, (1080, 1920), 48000, pix_fmt='uyvy422', colorspace='bt709', chroma_loc='left')
    feed = tracker.stream(ingest=ing)                           # raw frames (T, 1080, 1920, 2) uint8; y210: uint16; the others (T, 2 H, W)

Interlaced recordings (1080i50 / 1080i59.94 / 576i / 480i contribution feeds) are recordings of fields: field_order='tff' or 'bff' picks the one
field nearest each 25 fps slot and resizes it on its own to the frame's target size, its rows placed where they sit in the frame - no weave of two instants, no
deinterlacing filter (ops.ingest_video_fields, ops.ingest_video_planes_fields); fps_in stays the FRAME rate as ffprobe reports it; rgb24 and the 4:2:2 formats:

    ing = RecordingIngest(dev, (30000, 1001), (1080, 1920), 48000, pix_fmt='uyvy422', field_order='tff')

v210 is what SDI capture itself delivers for a 10-bit feed (DeckLink / AJA / Bluefish 10-bit YUV, QuickTime 'v210'): 4:2:2 in the uyvy422 order, three
10-bit samples per 32-bit word, six pixels per 16 bytes, rows padded to 128 bytes (v210_row_words).  It is read as it arrives (ops.ingest_video_v210, _fields):

    ing = RecordingIngest(dev, (30000, 1001), (1080, 1920), 48000, pix_fmt='v210', colorspace='bt709', field_order='tff')
    feed = tracker.stream(ingest=ing)                           # raw frames (T, 1080, 1280) int32: a byte buffer becomes this with .view(torch.int32)

Several audio programmes of one feed (an SDI / contribution feed carries up to 16 embedded channels - a stereo main mix, a second language, audio
description - each of which can be out of sync on its own) are tracked against ONE pass of the picture:

    ing = RecordingIngest(dev, 25, (1080, 1920), 48000, pix_fmt='uyvy422', audio_channels=8, audio_interleaved=True, programmes=[(0, 1), (2, 3), 4])
    tracks = tracker.track_raw_programmes(raw_frames, raw_wave, ing)      # raw_wave (n, 8) int16 / int32 (s24 left-justified) / fp32 -> one OffsetTrack per programme

Out of scope: decoding, 12-bit / 4:4:4 input through RecordingIngest (ops.ingest_video_planes takes a 4:4:4 planar layout), the 12-bit and 4:4:4 packed words (v410, r210), big-endian v210, deinterlacing filters, interlaced
4:2:0, a field order that changes mid-stream, telecine, BT.2020 in csc_matrix, transfer functions (PQ, HLG: a 10-bit HDR stream is converted by the matrix alone,
no tone mapping), double-buffered uploads, several recordings per call; for programmes: de-embedding, channel-layout metadata, loudness normalisation, more than
16 channels, u8 / packed s24 / float64 samples, per-programme sample rates or known delays.
"""
import math
from fractions import Fraction
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

CROP = 224                       # the model's input size; ops.INGEST_OUT and ops.INGEST_MAX_TAPS are these two
MAX_TAPS = 35                    # sf_ingest_video's range: a short side up to 2160 at resize_side 256
PIX_FMTS = ('rgb24', 'nv12', 'yuv420p', 'p010', 'yuv420p10le')
PIX_FMTS_16 = ('p010', 'yuv420p10le')   # 10-bit samples in uint16: ops.ingest_video_yuv16
PIX_FMTS_422 = ('uyvy422', 'yuyv422', 'yuv422p', 'nv16', 'yuv422p10le', 'p210', 'y210')     # 4:2:2: ops.ingest_video_planes
PIX_FMTS_422_16 = ('yuv422p10le', 'p210', 'y210')                                           # of those, 10-bit samples in uint16
PIX_FMTS_PACKED = ('uyvy422', 'yuyv422', 'y210')                                            # raw frames (T, H, W, 2): a macropixel Y0 U Y1 V (in some order) per two columns
PIX_FMTS_V210 = ('v210',)                                                                   # 10-bit 4:2:2, three samples per 32-bit word: ops.ingest_video_v210; raw frames (T, H, Pw) int32
FIELD_ORDERS = ('progressive', 'tff', 'bff')                                                   # frames; interlaced, top / bottom field first
MAX_AUDIO_CHANNELS = 16          # sf_resample_wave_mix's range (ops.MIX_MAX_CH)
WAVE_DTYPES = (torch.float32, torch.int16, torch.int32)                                        # of an ingest with programmes: flt, s16, s32 (s24 left-justified)
CHROMA_LOCS = {'center': (0.0, 0.0), 'left': (0.0, 0.25), 'topleft': (0.25, 0.25)}       # (shift of the cy tables, of the cx tables)
_KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


class PlaneLayout(NamedTuple):
    """Where the three planes of one frame lie: the arguments of sf_ingest_video_yuv_planes.  Strides and offsets in BYTES; the sample is a byte, or
    (word >> shift) & 1023 of a 16-bit word."""
    bytes_per_sample: int
    H: int
    W: int
    Hc: int
    Wc: int
    stride_frame: int
    y_off: int
    stride_row: int
    stride_col: int
    u_off: int
    v_off: int
    stride_crow: int
    stride_ccol: int
    shift: int


def plane_layout(pix_fmt: str, H: int, W: int, strides=None) -> PlaneLayout:
    """The PlaneLayout of raw frames of H x W in a named format: the seven 4:2:2 formats (PIX_FMTS_422) and the four 4:2:0 ones.  strides: the raw tensor's own
    strides in ELEMENTS (frame, row, column - or frame, row, column, 2 for the packed formats); None: contiguous.  A row pitch above W is taken where the format has
    one (packed, nv12 / nv16, p010 / p210); the planar formats are contiguous.  ValueError on an unknown name, odd W, odd H for 4:2:0, or strides the format cannot
    have.  The raw shapes: 4:2:0 (T, 3 H / 2, W); uyvy422 / yuyv422 / y210 (T, H, W, 2); the other 4:2:2 formats (T, 2 H, W)."""
    H, W = int(H), int(W)
    fmts = PIX_FMTS[1:] + PIX_FMTS_422
    if pix_fmt not in fmts:
        raise ValueError(f'plane_layout: pix_fmt = {pix_fmt!r}: one of {fmts}')
    is422 = pix_fmt in PIX_FMTS_422
    if H < 1 or W < 2 or W % 2 or (H % 2 and not is422):
        raise ValueError(f'plane_layout: {H} x {W} with pix_fmt = {pix_fmt!r}: {"4:2:2 takes even W" if is422 else "4:2:0 takes even H and W"}')
    b = 2 if pix_fmt in PIX_FMTS_16 + PIX_FMTS_422_16 else 1
    packed = pix_fmt in PIX_FMTS_PACKED
    rows = H if packed else 2 * H if is422 else 3 * H // 2
    if strides is None:
        strides = (rows * W * 2, W * 2, 2, 1) if packed else (rows * W, W, 1)
    strides = tuple(int(v) for v in strides)
    if len(strides) != (4 if packed else 3) or strides[0] < 0:
        raise ValueError(f'plane_layout: {pix_fmt} frames with strides {strides}')
    sf, sy = strides[0], strides[1]
    pitched = packed or pix_fmt in ('nv12', 'nv16', 'p010', 'p210')
    if strides[2:] != ((2, 1) if packed else (1,)) or (sy < (2 * W if packed else W) if pitched else sy != W):
        raise ValueError(f'plane_layout: {pix_fmt} frames with strides {strides}: '
                         + ('inner strides (2, 1) and a row stride of at least 2 W expected' if packed else
                            'unit column stride and ' + ('a row stride of at least W' if pitched else 'contiguous rows') + ' expected'))
    P = sy * b                                                                    # the row pitch in bytes
    Hc = H if is422 else H // 2
    shift = 6 if pix_fmt in ('p010', 'p210', 'y210') else 0
    if packed:                                                                    # y_off, u_off, v_off inside the macropixel, in samples
        yo, uo, vo = (1, 0, 2) if pix_fmt == 'uyvy422' else (0, 1, 3)
        return PlaneLayout(b, H, W, Hc, W // 2, sf * b, yo * b, P, 2 * b, uo * b, vo * b, P, 4 * b, shift)
    if pitched:                                                                   # H luma rows, then the rows of interleaved U V
        return PlaneLayout(b, H, W, Hc, W // 2, sf * b, 0, P, b, P * H, P * H + b, P, 2 * b, shift)
    return PlaneLayout(b, H, W, Hc, W // 2, sf * b, 0, P, b, H * W * b, (H * W + Hc * (W // 2)) * b, (W // 2) * b, b, shift)


def v210_row_words(W: int, aligned: bool = True) -> int:
    """The 32-bit words of a v210 row of W pixels: 32 ceil(W / 48), the conventional pitch of 128 ceil(W / 48) bytes (1920 -> 1280 words, 1280 -> 864, 720 -> 480);
    aligned=False: the 4 ceil(W / 6) words that hold samples (whole groups of six pixels), the least a row can have."""
    W = int(W)
    if W < 1:
        raise ValueError(f'v210_row_words: W = {W}')
    return 32 * -(-W // 48) if aligned else 4 * -(-W // 6)


def _fraction(fps) -> Fraction:
    if isinstance(fps, (tuple, list)):
        if len(fps) != 2:
            raise ValueError(f'fps = {fps}: expected a number or a (num, den) pair')
        f = Fraction(int(fps[0]), int(fps[1]))
    elif isinstance(fps, float):
        f = Fraction(fps).limit_denominator(1001)
    else:
        f = Fraction(fps)
    if f <= 0:
        raise ValueError(f'fps = {fps}')
    return f


def fps_frame_table(n_in: int, fps_in, fps_out=25) -> torch.Tensor:
    """Which source frame each output frame shows when `n_in` frames at `fps_in` are converted to `fps_out`: int32 (T_out,).
    fps_in / fps_out: an int, a float (taken as Fraction(fps).limit_denominator(1001): 29.97 -> 30000/1001) or a (num, den) pair; exact rational arithmetic.
    The rule is the default rounding ("near") of ffmpeg's fps filter as documented: source frame i lands on output slot
    p_i = floor(i * fps_out / fps_in + 1/2) (half away from zero for i >= 0), the output has T_out = p_{n_in - 1} + 1 frames, and slot j shows the last source
    frame that landed at or before it, src[j] = max{i : p_i <= j} (frames that share a slot are dropped but the last, empty slots repeat).
    This RESTATES the documented rule; parity with a particular ffmpeg build (its end-of-stream handling in particular) cannot be checked here and is not claimed."""
    fi, fo = _fraction(fps_in), _fraction(fps_out)
    n_in = int(n_in)
    if n_in <= 0:
        return torch.empty(0, dtype=torch.int32)
    if fi == fo:
        return torch.arange(n_in, dtype=torch.int32)
    r = fo / fi
    half = Fraction(1, 2)
    slots = [math.floor(i * r + half) for i in range(n_in)]                      # non-decreasing
    src = [0] * (slots[-1] + 1)
    i = 0
    for j in range(len(src)):
        while i + 1 < n_in and slots[i + 1] <= j:
            i += 1
        src[j] = i
    return torch.tensor(src, dtype=torch.int32)


def fps_field_table(n_frames: int, fps_in, fps_out=25) -> torch.Tensor:
    """Which FIELD each output frame shows when n_frames interlaced frames at frame rate fps_in are converted to fps_out: an interlaced recording is a progressive
    one of 2 n_frames fields at 2 fps_in, so this is fps_frame_table(2 n_frames, 2 fps_in, fps_out) - the same "near" rule.  Field f is temporal: the first field
    of frame f >> 1 when f is even, whichever rows the field order gives it.  At 25i: 0, 2, 4, .. and the end-of-stream slot; at 30000/1001 the parities alternate."""
    return fps_frame_table(2 * int(n_frames), 2 * _fraction(fps_in), fps_out)


def resized_dims(H: int, W: int, side: int = 256) -> Tuple[int, int]:
    """(Hr, Wr) after `scale=-2:side` / `side:-2` style resizing of example.py:16-53: the short side becomes `side`, the other one d * side // short, cut to even."""
    H, W, side = int(H), int(W), int(side)
    if H < 1 or W < 1 or side < 1:
        raise ValueError(f'resized_dims: {H} x {W} to side {side}')
    if H <= W:
        return side, (W * side // H) // 2 * 2
    return (H * side // W) // 2 * 2, side


def _cubic(x: torch.Tensor, a: float = -0.5) -> torch.Tensor:
    x = x.abs()
    near = ((a + 2) * x - (a + 3)) * x * x + 1
    far = ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
    return torch.where(x < 1, near, torch.where(x < 2, far, torch.zeros_like(x)))


def aa_bicubic_table(n_in: int, n_out: int, dtype=torch.float32, shift: float = 0.0):
    """The separable filter of F.interpolate(mode='bicubic', antialias=True, align_corners=False) along one axis, n_in -> n_out samples (cubic a = -0.5):
    (first int32 (n_out,), weights fp32 (n_out, taps), taps) with out[i] = sum_j weights[i, j] * in[first[i] + j].  scale = n_in / n_out; when downscaling the
    kernel is stretched by scale (support 2 scale), otherwise support 2; taps = 2 ceil(support) + 1; rows are normalised to sum 1 in float64, stored fp32,
    zero-padded to `taps` (first[i] + j may then pass n_in - 1: those weights are zero).  At scale 1 it is the identity.  dtype=torch.float64 returns the weights
    before the fp32 rounding (for checks of the formula itself).  shift moves the filter centre, c = scale (i + 0.5) + shift in source samples: source sample j is
    taken to sit at coordinate j + 0.5, so a chroma sample co-sited with luma sample 2 k (luma coordinate 2 k + 0.5 = chroma coordinate k + 0.25) asks for
    shift=0.25; 0.0 is F.interpolate's own geometry."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f'aa_bicubic_table: {n_in} -> {n_out}')
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    taps = 2 * math.ceil(support) + 1
    first = torch.zeros(n_out, dtype=torch.int32)
    w = torch.zeros(n_out, taps, dtype=torch.float64)
    j = torch.arange(taps, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5) + shift
        xmin = max(0, int(c - support + 0.5))
        xsize = min(n_in, int(c + support + 0.5)) - xmin
        row = _cubic((j[:xsize] + xmin - c + 0.5) * inv)
        first[i] = xmin
        w[i, :xsize] = row / row.sum()
    return first, w.to(dtype), taps


def _crop_table(n_in: int, n_out: int, origin: int, crop: int, dev, shift: float = 0.0):
    """aa_bicubic_table(n_in, n_out, shift=shift) cut to the output samples [origin, origin + crop), on the device: (first, weights, taps)."""
    first, w, taps = aa_bicubic_table(n_in, n_out, shift=shift)
    return first[origin:origin + crop].contiguous().to(dev), w[origin:origin + crop].contiguous().to(dev), taps


def csc_matrix(colorspace: str = 'bt601', full_range: bool = False, bit_depth: int = 8):
    """(M (3, 3) float64, offsets (3,) float64) with (R, G, B) = M @ ((Y, U, V) - offsets): samples on the `bit_depth` scale (8 or 10), RGB on the 8-bit scale.
    On the 8-bit scale, with Kr, Kb of the colour space (bt601: 0.299,
    0.114; bt709: 0.2126, 0.0722), Kg = 1 - Kr - Kb, luma gain gy and chroma gain gc (limited range: 255 / 219 and 255 / 224, offsets (16, 128, 128); full range:
    1 and 1, offsets (0, 128, 128)):  R = gy Y' + 2 (1 - Kr) gc V',  B = gy Y' + 2 (1 - Kb) gc U',  G = gy Y' - 2 Kb (1 - Kb) / Kg gc U' - 2 Kr (1 - Kr) / Kg gc V'.
    bit_depth=10: limited range has gains 255 / (219 * 4) and 255 / (224 * 4), offsets (64, 512, 512) - the 8-bit matrix divided by 4, exactly; full range has
    gains 255 / 1023, offsets (0, 512, 512)."""
    if colorspace not in _KR_KB:
        raise ValueError(f'colorspace = {colorspace!r}: one of {sorted(_KR_KB)}')
    if bit_depth not in (8, 10):
        raise ValueError(f'bit_depth = {bit_depth}: 8 or 10')
    kr, kb = _KR_KB[colorspace]
    kg = 1.0 - kr - kb
    gy, gc, o0 = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    oc = 128.0
    if bit_depth == 10:                                                          # a power of two: every entry of the limited-range matrix is the 8-bit one / 4
        gy, gc = (255.0 / 1023.0, 255.0 / 1023.0) if full_range else (gy / 4.0, gc / 4.0)
        o0, oc = 4.0 * o0, 512.0
    M = torch.tensor([[gy, 0.0, 2 * (1 - kr) * gc],
                      [gy, -2 * kb * (1 - kb) / kg * gc, -2 * kr * (1 - kr) / kg * gc],
                      [gy, 2 * (1 - kb) * gc, 0.0]], dtype=torch.float64)
    return M, torch.tensor([o0, oc, oc], dtype=torch.float64)


def programme_matrix(programmes: Sequence, n_channels: int) -> torch.Tensor:
    """The down-mix of a multi-channel wave into audio programmes: fp32 (P, n_channels), row p the weights of programme p.  A programme is an int (that
    channel, weight 1), a tuple / list of ints (those channels at equal weights 1 / k: a stereo pair averaged as sf_resample_wave averages) or a dict
    {channel: weight}.  ValueError on an empty list, an empty programme, a channel outside [0, n_channels), a channel named twice in one programme, a non-finite
    weight."""
    n_channels = int(n_channels)
    if isinstance(programmes, (int, dict)) or programmes is None or len(programmes) == 0:
        raise ValueError(f'programme_matrix: programmes = {programmes!r}: a non-empty list of programmes')
    if n_channels < 1:
        raise ValueError(f'programme_matrix: n_channels = {n_channels}')
    M = torch.zeros(len(programmes), n_channels, dtype=torch.float32)
    for p, prog in enumerate(programmes):
        if isinstance(prog, dict):
            items = list(prog.items())
        elif isinstance(prog, (tuple, list)):
            items = [(c, 1.0 / len(prog)) for c in prog]
        elif isinstance(prog, int) and not isinstance(prog, bool):
            items = [(prog, 1.0)]
        else:
            raise ValueError(f'programme_matrix: programme {p} = {prog!r}: an int, a tuple of ints or a dict {{channel: weight}}')
        if not items:
            raise ValueError(f'programme_matrix: programme {p} is empty')
        seen = set()
        for c, w in items:
            if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < n_channels:
                raise ValueError(f'programme_matrix: programme {p} names channel {c!r}, the wave has channels 0 .. {n_channels - 1}')
            if c in seen:
                raise ValueError(f'programme_matrix: programme {p} names channel {c} twice')
            if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w):
                raise ValueError(f'programme_matrix: programme {p}, channel {c}: weight {w!r} is not a finite number')
            seen.add(c)
            M[p, c] = float(w)
    return M


def resample_kernel(rate_in: int, rate_out: int = 16000, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The polyphase windowed-sinc bank of torchaudio.functional.resample at its defaults (sinc_interp_hann): (kernel fp32 (n, 2 width + o), width, o, n) with
    o = rate_in / gcd, n = rate_out / gcd.  Output y[p + n q] = sum_i xpad[q o + i] * kernel[p, i] on x zero-padded by (width, width + o), cut to
    ceil(n len / o) samples.  The filter is centred on the output sample's own time: no delay (a sync model cannot tolerate one)."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError(f'resample_kernel: {rate_in} -> {rate_out} Hz')
    g = math.gcd(rate_in, rate_out)
    o, n = rate_in // g, rate_out // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64) / o
    t = (-torch.arange(n, dtype=torch.float64)[:, None] / n + idx[None]) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    win = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    tp = t * math.pi
    sinc = torch.where(tp == 0, torch.ones_like(tp), tp.sin() / torch.where(tp == 0, torch.ones_like(tp), tp))
    return (sinc * win * (base / o)).float(), width, o, n


class RecordingIngest:
    """The geometry of one kind of recording, tables on the device, built once.
    fps_in: int, float or (num, den); size_in = (H, W) of the raw frames; rate_in: Hz; channels_last: raw frames are (T, H, W, 3) as decoders hand them out,
    otherwise planar (T, 3, H, W); resize_side: what the short side is scaled to (256, the even cut of the other side as in example.py); crop stays 224, centred
    with RGBSpatialCrop's origin int(round((Hr - 224) / 2.)).  pix_fmt: 'rgb24' (the layouts above), or 'nv12' / 'yuv420p': raw frames are (T, 3 H / 2, W), 8-bit
    YUV 4:2:0 (ops.ingest_video_yuv), or 'p010' / 'yuv420p10le': the same shape in uint16 (int16 is read as the same bits), 10-bit YUV 4:2:0
    (ops.ingest_video_yuv16), or one of PIX_FMTS_422: 4:2:2 (ops.ingest_video_planes) - 'uyvy422' / 'yuyv422' uint8 (T, H, W, 2), a pitched view read in place
    (inner strides 2, 1); 'y210' the same in uint16; 'nv16' uint8 / 'p210' uint16 (T, 2 H, W) at any row pitch; 'yuv422p' uint8 / 'yuv422p10le' uint16 (T, 2 H, W)
    contiguous; 'v210'  int32 / uint32 (T, H, Pw), Pw >= 4 ceil(W / 6) words at any row pitch (v210_row_words), interlaced too; even W only, an odd H is legal; the chroma rows take the luma tables, so 'topleft' is 'left' - converted with csc_matrix(colorspace, full_range, bit_depth) after the resize, or with csc = (M (3, 3), offsets (3,)) on the format's
    own sample scale when given (it overrides colorspace / full_range; e.g. BT.2020 coefficients).  chroma_loc: 'center', 'left' or 'topleft' (CHROMA_LOCS; YUV
    formats only).  ValueError on resize_side < crop, crop != 224, a source so large that a filter row passes 35 taps (short side above ~2160 at resize_side 256),
    an unknown pix_fmt, colorspace or chroma_loc, chroma_loc or csc with rgb24, and for a YUV format odd H or W or channels_last=True.
    field_order: 'progressive' (the default: frames), or 'tff' / 'bff' (DESIGN 3.18): the raw frames are interlaced, top / bottom field first, fps_in is still the
    frame rate.  The recording is then its 2 n fields at 2 fps_in: frame_table / n_frames come from fps_field_table, every output frame is ONE field resized to the
    frame's (Hr, Wr) with the vertical table of its parity p, aa_bicubic_table(H / 2, Hr, shift = 0.25 - p / 2) (y_tables; 4:2:2 chroma rows take the same two), and
    the 35-tap limit applies to the field's taps.  ValueError on an unknown field_order, an odd H with an interlaced order, or an interlaced order with a 4:2:0 format
    (field-sited chroma is another geometry).
    programmes: a list for programme_matrix - the wave then has audio_channels channels (1 .. 16), planar (ch, n) or, with audio_interleaved, (n, ch),
    fp32, int16 or int32 (s24 left-justified), and .waves() gives one 16 kHz wave per programme from one read of the input (ops.resample_wave_mix); .wave() raises.
    programmes=None (the default) is the object without them: no attribute changes.  ValueError on audio_channels / audio_interleaved without programmes,
    audio_channels outside 1 .. 16, and whatever programme_matrix refuses."""

    field_order, interlaced = 'progressive', False
    programmes = None

    def __init__(self, device, fps_in, size_in, rate_in: int, channels_last: bool = False, resize_side: int = 256, crop: int = CROP, pix_fmt: str = 'rgb24',
                 colorspace: str = 'bt601', full_range: bool = False, chroma_loc: str = 'center', csc=None, field_order: str = 'progressive',
                 audio_channels: Optional[int] = None, audio_interleaved: bool = False, programmes=None):
        if programmes is None:
            if audio_channels is not None or audio_interleaved:
                raise ValueError('audio_channels / audio_interleaved describe the wave of an ingest with programmes: pass programmes=[...]')
        else:
            if audio_channels is None or isinstance(audio_channels, bool) or not 1 <= int(audio_channels) <= MAX_AUDIO_CHANNELS:
                raise ValueError(f'audio_channels = {audio_channels!r} with programmes: the channels of the wave, 1 .. {MAX_AUDIO_CHANNELS}')
            mix = programme_matrix(programmes, int(audio_channels))
        if field_order not in FIELD_ORDERS:
            raise ValueError(f'field_order = {field_order!r}: one of {FIELD_ORDERS}')
        if pix_fmt not in PIX_FMTS + PIX_FMTS_422 + PIX_FMTS_V210:
            raise ValueError(f'pix_fmt = {pix_fmt!r}: one of {PIX_FMTS + PIX_FMTS_422 + PIX_FMTS_V210}')
        if chroma_loc not in CHROMA_LOCS:
            raise ValueError(f'chroma_loc = {chroma_loc!r}: one of {tuple(CHROMA_LOCS)}')
        if pix_fmt == 'rgb24' and (chroma_loc != 'center' or csc is not None):
            raise ValueError(f"chroma_loc = {chroma_loc!r} / csc with pix_fmt = 'rgb24': they describe YUV frames")
        if colorspace not in _KR_KB:
            raise ValueError(f'colorspace = {colorspace!r}: one of {sorted(_KR_KB)}')
        if crop != CROP:
            raise ValueError(f'crop = {crop}: the model takes {CROP} x {CROP} frames')
        if resize_side < crop:
            raise ValueError(f'resize_side = {resize_side} below the {crop} crop')
        self.dev = torch.device(device)
        self.fps_in, self.rate_in, self.channels_last = _fraction(fps_in), int(rate_in), bool(channels_last)
        self.H, self.W = int(size_in[0]), int(size_in[1])
        if field_order != 'progressive':                                          # (a progressive object keeps the attributes it had: the class holds the defaults)
            self.field_order, self.interlaced = field_order, True
        if self.interlaced and pix_fmt != 'rgb24' and pix_fmt not in PIX_FMTS_422 + PIX_FMTS_V210:
            raise ValueError(f'field_order = {field_order!r} with pix_fmt = {pix_fmt!r}: interlaced 4:2:0 (field-sited chroma) is out of scope; rgb24 or one of '
                             f'{PIX_FMTS_422 + PIX_FMTS_V210}')
        if self.interlaced and (self.H % 2 or self.H < 2):
            raise ValueError(f'field_order = {field_order!r} with H = {self.H}: two fields take an even H')
        self.Hr, self.Wr = resized_dims(self.H, self.W, resize_side)
        if self.Hr < crop or self.Wr < crop:
            raise ValueError(f'{self.H} x {self.W} resizes to {self.Hr} x {self.Wr}, below the {crop} crop')
        self.y0, self.x0 = int(round((self.Hr - crop) / 2.)), int(round((self.Wr - crop) / 2.))
        if self.interlaced:
            # a field's H / 2 rows to the FRAME's Hr: row k of the field of parity p is frame row 2 k + p, centre 2 k + p + 0.5 = 2 (k + 0.5 + 0.25 - p / 2)
            tabs = [_crop_table(self.H // 2, self.Hr, self.y0, crop, self.dev, 0.25 - p / 2) for p in (0, 1)]
            self.y_tables, self.taps_y = tuple(t[:2] for t in tabs), tabs[0][2]       # one tap count: the scale is the same
            self.y_first, self.y_w = self.y_tables[0]
        else:
            self.y_first, self.y_w, self.taps_y = _crop_table(self.H, self.Hr, self.y0, crop, self.dev)
        self.x_first, self.x_w, self.taps_x = _crop_table(self.W, self.Wr, self.x0, crop, self.dev)
        if max(self.taps_y, self.taps_x) > MAX_TAPS:
            raise ValueError(f'{self.H} x {self.W} -> {self.Hr} x {self.Wr} needs {self.taps_y} x {self.taps_x} filter taps, the kernel takes {MAX_TAPS} '
                             f'(a short side up to 2160 at 256)')
        self.pix_fmt = pix_fmt
        if pix_fmt != 'rgb24':
            v210 = pix_fmt in PIX_FMTS_V210
            is422 = pix_fmt in PIX_FMTS_422 or v210                                   # (v210 is 4:2:2 for every table below)
            if channels_last:
                raise ValueError(f'channels_last=True with pix_fmt = {pix_fmt!r}: a YUV frame is '
                                 f'{"(H, words per row)" if v210 else "(H, W, 2)" if pix_fmt in PIX_FMTS_PACKED else "(2 H, W)" if is422 else "(3 H / 2, W)"}')
            if self.W % 2 or (self.H % 2 and not is422):
                raise ValueError(f'{self.H} x {self.W} with pix_fmt = {pix_fmt!r}: {"4:2:2 takes even W" if is422 else "4:2:0 takes even H and W"}')
            # chroma: an (H / 2, W / 2) image resized to the same (Hr, Wr), sliced at the same crop origin; never more taps than luma
            # chroma_loc: the quarter-sample shift of sited chroma goes into these tables, the kernels never see it
            self.chroma_loc = chroma_loc
            # 4:2:2 has no vertical subsampling: the chroma rows are the luma rows, the luma tables serve them and 'topleft' is 'left'
            self.cy_first, self.cy_w, self.taps_cy = (self.y_first, self.y_w, self.taps_y) if is422 else \
                _crop_table(self.H // 2, self.Hr, self.y0, crop, self.dev, CHROMA_LOCS[chroma_loc][0])
            self.cx_first, self.cx_w, self.taps_cx = _crop_table(self.W // 2, self.Wr, self.x0, crop, self.dev, CHROMA_LOCS[chroma_loc][1])
            self.colorspace, self.full_range = colorspace, bool(full_range)
            if csc is None:
                M, off = csc_matrix(colorspace, full_range, 10 if pix_fmt in PIX_FMTS_16 + PIX_FMTS_422_16 + PIX_FMTS_V210 else 8)
            else:
                M, off = (torch.as_tensor(v, dtype=torch.float64).cpu() for v in csc)
                if M.shape != (3, 3) or off.shape != (3,):
                    raise ValueError(f'csc: expected (M (3, 3), offsets (3,)), got {tuple(M.shape)} and {tuple(off.shape)}')
            self.csc = torch.cat([M.reshape(9), off]).float()                        # host: the twelve floats travel as kernel arguments
        if self.rate_in == 16000:
            self.kernel, self.width, self.o, self.n = torch.ones(1, 1), 0, 1, 1   # down-mix / PCM scaling only
        else:
            self.kernel, self.width, self.o, self.n = resample_kernel(self.rate_in)
        self.kernel = self.kernel.contiguous().to(self.dev)
        self._tables = {}
        if programmes is not None:                                               # (an object without programmes keeps the attributes it had)
            self.programmes, self.audio_channels, self.audio_interleaved = list(programmes), int(audio_channels), bool(audio_interleaved)
            self.mix = mix.to(self.dev)

    def frame_table(self, n_in: int) -> torch.Tensor:
        """fps_frame_table(n_in, fps_in) (host, cached per n_in); interlaced: fps_field_table(n_in, fps_in), FIELD indices."""
        if n_in not in self._tables:
            self._tables = {n_in: (fps_field_table if self.interlaced else fps_frame_table)(n_in, self.fps_in)}
        return self._tables[n_in]

    def n_frames(self, n_in: int) -> int:
        """25 fps frames that n_in raw frames give."""
        return int(self.frame_table(n_in).numel())

    def n_samples(self, n_in: int) -> int:
        """16 kHz samples that n_in raw samples give: ceil(n * n_in / o)."""
        return -(-self.n * int(n_in) // self.o)

    def _check_frames(self, raw: torch.Tensor):
        if self.pix_fmt in PIX_FMTS_V210:
            need = v210_row_words(self.W, aligned=False)
            if raw.dim() != 3 or raw.dtype not in (torch.int32, torch.uint32) or raw.shape[1] != self.H or raw.shape[2] < need:
                raise ValueError(f'raw frames: expected int32 (T, {self.H}, Pw >= {need}) - v210 words, four per six pixels; a byte buffer becomes this with '
                                 f'.view(torch.int32) - got {raw.dtype} {tuple(raw.shape)}')
            return
        want = (self.H, self.W, 2) if self.pix_fmt in PIX_FMTS_PACKED else (2 * self.H, self.W) if self.pix_fmt in PIX_FMTS_422 else \
            (self.H * 3 // 2, self.W) if self.pix_fmt != 'rgb24' else (self.H, self.W, 3) if self.channels_last else (3, self.H, self.W)
        dtypes = (torch.uint16, torch.int16) if self.pix_fmt in PIX_FMTS_16 + PIX_FMTS_422_16 else (torch.uint8,)
        if raw.dim() != len(want) + 1 or raw.dtype not in dtypes or tuple(raw.shape[1:]) != want:
            raise ValueError(f'raw frames: expected {str(dtypes[0])[6:]} (T, {", ".join(map(str, want))}), got {raw.dtype} {tuple(raw.shape)}')

    def frames(self, raw: torch.Tensor, j0: int, j1: int) -> torch.Tensor:
        """25 fps frames [j0, j1) of the recording, resized and cropped: uint8 (j1 - j0, 3, 224, 224) on the device.  raw: all the raw frames, device or host; from
        a host tensor only the source frames frame_table[j0:j1] spans are uploaded (interlaced: the frames that hold the fields it spans)."""
        self._check_frames(raw)
        table = self.frame_table(raw.shape[0])
        if not 0 <= j0 <= j1 <= table.numel():
            raise ValueError(f'frames [{j0}, {j1}) of {table.numel()}')
        if j1 == j0:
            return torch.empty(0, 3, CROP, CROP, device=self.dev, dtype=torch.uint8)
        t = table[j0:j1]
        u = 2 if self.interlaced else 1                                          # table entries per source frame
        lo, hi = int(t[0]) // u, int(t[-1]) // u + 1                             # the table is non-decreasing
        return self._resize(raw[lo:hi].to(self.dev, non_blocking=True), t - u * lo)

    def _resize(self, src: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """Output frame j = source frame src[t[j]] (src on the device, t int32 on the host), resized and cropped; interlaced: field t[j] of src's 2 len(src) fields."""
        from . import ops
        table, bff = t.to(self.dev, non_blocking=True), self.field_order == 'bff'
        y, x = (self.y_first, self.y_w), (self.x_first, self.x_w)
        if self.pix_fmt == 'rgb24':
            if self.interlaced:
                return ops.ingest_video_fields(src, self.channels_last, table, self.y_tables, *x, bff)
            return ops.ingest_video(src, self.channels_last, table, *y, *x)
        cy, cx = (self.cy_first, self.cy_w), (self.cx_first, self.cx_w)
        if self.pix_fmt in PIX_FMTS_V210:
            if self.interlaced:
                return ops.ingest_video_v210_fields(src, self.W, table, self.y_tables, *x, *cx, self.csc, bff)
            return ops.ingest_video_v210(src, self.W, table, *y, *x, *cx, self.csc)
        if self.pix_fmt in PIX_FMTS_422:                                         # (the only YUV formats an interlaced ingest takes)
            layout = plane_layout(self.pix_fmt, self.H, self.W, src.stride())
            if self.interlaced:
                return ops.ingest_video_planes_fields(src, layout, table, self.y_tables, *x, self.y_tables, *cx, self.csc, bff)
            return ops.ingest_video_planes(src, layout, table, *y, *x, *cy, *cx, self.csc)
        op = ops.ingest_video_yuv16 if self.pix_fmt in PIX_FMTS_16 else ops.ingest_video_yuv
        return op(src, self.pix_fmt, table, *y, *x, *cy, *cx, self.csc)

    def wave(self, raw_wave: torch.Tensor) -> torch.Tensor:
        """raw_wave (n,) or (ch, n), fp32 or int16 PCM, device or host -> mono fp32 16 kHz (n16k,) on the device.  A mono fp32 wave at 16 kHz is returned as it is."""
        if self.programmes is not None:
            raise ValueError(f'RecordingIngest.wave: this ingest has {len(self.programmes)} programmes, there is no single wave: use .waves()')
        if raw_wave.dim() not in (1, 2) or raw_wave.dtype not in (torch.float32, torch.int16) or (raw_wave.dim() == 2 and not 1 <= raw_wave.shape[0] <= 8):
            raise ValueError(f'raw wave: expected fp32 or int16 (n,) or (ch <= 8, n), got {raw_wave.dtype} {tuple(raw_wave.shape)}')
        x = raw_wave.to(self.dev, non_blocking=True)
        if self.rate_in == 16000 and x.dtype == torch.float32 and (x.dim() == 1 or x.shape[0] == 1):
            return x.reshape(-1)
        from . import ops
        return ops.resample_wave(x, self.kernel, self.o, self.width)

    def _check_wave(self, raw_wave: torch.Tensor):
        ch = self.audio_channels
        want = ('n', ch) if self.audio_interleaved else (ch, 'n')
        if raw_wave.dim() != 2 or raw_wave.dtype not in WAVE_DTYPES or raw_wave.shape[0 if not self.audio_interleaved else 1] != ch:
            raise ValueError(f'raw wave: expected fp32, int16 or int32 ({want[0]}, {want[1]}), got {raw_wave.dtype} {tuple(raw_wave.shape)}')

    def waves(self, raw_wave: torch.Tensor, len_out: Optional[int] = None) -> torch.Tensor:
        """The programmes of a multi-channel wave: raw_wave fp32, int16 or int32 (s24 left-justified), (audio_channels, n), or (n, audio_channels) when
        audio_interleaved, device or host -> fp32 16 kHz (P, n16k) on the device, row p the programme programmes[p].  One read of the input.  At 16 kHz the identity
        bank goes through the same kernel: the rows are the mix itself, to the last bit."""
        if self.programmes is None:
            raise ValueError('RecordingIngest.waves: this ingest has no programmes: use .wave()')
        self._check_wave(raw_wave)
        from . import ops
        return ops.resample_wave_mix(raw_wave.to(self.dev, non_blocking=True), self.mix, self.kernel, self.o, self.width, self.audio_interleaved, len_out)

    def stream(self) -> 'IngestStream':
        """The same conversion for a recording that is still arriving: see IngestStream."""
        return IngestStream(self)


def fps_final_slots(n_in: int, fps_in, fps_out=25) -> int:
    """How many output slots of fps_frame_table are FINAL once n_in source frames have been seen: slot j is final when a source frame with p_i > j has arrived,
    so slots [0, p_{n_in - 1}) are (the table of a prefix equals the table of the whole recording except in its last slot).  0 for n_in = 0."""
    if n_in <= 0:
        return 0
    return math.floor((n_in - 1) * (_fraction(fps_out) / _fraction(fps_in)) + Fraction(1, 2))


def fps_slot_source(j: int, fps_in, fps_out=25) -> int:
    """The source frame of a final slot j: max{i : floor(i r + 1/2) <= j} = ceil((j + 1/2) / r) - 1, exact rational arithmetic (r = fps_out / fps_in)."""
    return math.ceil((j + Fraction(1, 2)) / (_fraction(fps_out) / _fraction(fps_in))) - 1


def resample_stream_plan(emitted: int, seen: int, o: int, width: int, n: int, final: bool = False):
    """The resampler of a stream: `emitted` output samples are out (a multiple of n), `seen` raw samples have arrived.  -> (c0, k0, k1, hold): run the offline
    resampler on raw[c0:seen] and take its outputs [k0, k1): they are the recording's outputs [emitted, emitted + k1 - k0); afterwards the raw samples before
    `hold` are never read again.  Output p + n q reads raw samples [q o - width, q o + width + o): c0 is a multiple of o at most (emitted / n) o - width (0 while
    the filter still reaches before the recording: the zero padding there is the offline one), so the chunk's polyphase grid is the recording's, and an output
    is taken only when all its taps have arrived - or at the end (final), where the offline call zero-pads on the right and cuts at ceil(n seen / o)."""
    q_next = emitted // n
    c0 = max(0, (q_next * o - width) // o) * o
    if final:
        k1 = -(-n * seen // o) - n * (c0 // o)
    else:
        q_end = max(q_next, (seen - width - o) // o + 1 if seen >= width + o else 0)      # groups q < q_end have every tap inside [0, seen)
        k1 = n * q_end - n * (c0 // o)
    k0 = emitted - n * (c0 // o)
    done = emitted + k1 - k0
    return c0, k0, k1, max(0, ((done // n) * o - width) // o) * o


class IngestStream:
    """RecordingIngest for a feed: push(raw_frames, raw_wave) and flush() return the 25 fps frames (uint8 (t, 3, 224, 224)) and the 16 kHz samples (fp32 (m,)) that
    have become FINAL, on the device; concatenated over all calls they are bit-equal to ingest.frames(raw_all, 0, n_frames) and ingest.wave(raw_all), for every
    chunking.  An interlaced ingest counts fields (two per frame seen) and still holds one source FRAME.  Host logic over the same kernels: the last source frame is held until a later one shows which slots it fills (flush emits its slot), the raw
    samples are held from the resampler's left context on (resample_stream_plan).  Either argument may be empty (or None).  An ingest with programmes
    holds the raw samples in the layout they arrive in, (ch, m) or (m, ch), returns fp32 (P, m) per call, and the concatenation along the samples is bit-equal to
    ingest.waves(raw_all); the plan, and so the bound on the held samples, is the same."""

    def __init__(self, ingest: RecordingIngest):
        self.ing = ingest
        self.n_src = self.slots_out = 0          # source frames seen, 25 fps frames emitted
        self._last = None                        # the last source frame, on the device (1, ...)
        self.raw_seen = self.samples_out = 0     # raw samples seen, 16 kHz samples emitted
        self._raw = None                         # raw samples [self._raw0, raw_seen) on the device, (ch, m)
        self._raw0 = 0
        self._t = 0 if ingest.programmes is not None and ingest.audio_interleaved else 1      # the sample axis of the held raw wave
        self.closed = False

    @property
    def held(self) -> dict:
        return dict(frames=0 if self._last is None else 1, samples=0 if self._raw is None else int(self._raw.shape[self._t]))

    def _passthrough(self, x: torch.Tensor) -> bool:
        return self.ing.rate_in == 16000 and x.dtype == torch.float32 and x.shape[0] == 1

    def push(self, raw_frames: Optional[torch.Tensor] = None, raw_wave: Optional[torch.Tensor] = None):
        if self.closed:
            raise RuntimeError('IngestStream.push: the stream was closed by flush()')
        return self._frames(raw_frames, False), self._wave(raw_wave, False)

    def flush(self):
        if self.closed:
            raise RuntimeError('IngestStream.flush: the stream is closed')
        self.closed = True
        return self._frames(None, True), self._wave(None, True)

    def _frames(self, raw: Optional[torch.Tensor], final: bool) -> torch.Tensor:
        ing = self.ing
        src, base = self._last, self.n_src - 1                                    # src[k] = source frame base + k
        if raw is not None and raw.shape[0]:
            ing._check_frames(raw)
            new = raw.to(ing.dev, non_blocking=True)
            new = new.view(torch.int16) if new.dtype == torch.uint16 else new.view(torch.int32) if new.dtype == torch.uint32 else new     # (the same bits; the kernels read either)
            src, base = (new, self.n_src) if src is None else (torch.cat([src, new]), base)
            self.n_src += int(raw.shape[0])
        u = 2 if ing.interlaced else 1                                            # an interlaced frame is two fields at twice the rate: the slots are the fields'
        j1 = fps_final_slots(u * self.n_src, u * ing.fps_in) + (1 if final and self.n_src else 0)
        j0, self.slots_out = self.slots_out, max(j1, self.slots_out)
        if src is not None:
            self._last = src[-1:].clone() if not final else None
        if j1 <= j0:
            return torch.empty(0, 3, CROP, CROP, device=ing.dev, dtype=torch.uint8)
        t = torch.tensor([min(fps_slot_source(j, u * ing.fps_in), u * self.n_src - 1) - u * base for j in range(j0, j1)], dtype=torch.int32)
        return ing._resize(src, t)

    def _waves(self, raw: Optional[torch.Tensor], final: bool) -> torch.Tensor:
        """_wave for an ingest with programmes: the same plan over the raw samples as they arrive, P rows out."""
        ing, t = self.ing, self._t
        if raw is not None and raw.shape[t if raw.dim() == 2 else 0]:
            ing._check_wave(raw)
            x = raw.to(ing.dev, non_blocking=True)
            self._raw = x if self._raw is None else torch.cat([self._raw, x], t)
            self.raw_seen += int(x.shape[t])
        P = len(ing.programmes)
        if self._raw is None:
            return torch.empty(P, 0, device=ing.dev, dtype=torch.float32)
        c0, k0, k1, hold = resample_stream_plan(self.samples_out, self.raw_seen, ing.o, ing.width, ing.n, final)
        out = torch.empty(P, 0, device=ing.dev, dtype=torch.float32)
        if k1 > k0:
            out = ing.waves(self._raw.narrow(t, c0 - self._raw0, self.raw_seen - c0), len_out=k1)[:, k0:]
            self.samples_out += k1 - k0
        self._raw, self._raw0 = self._raw.narrow(t, hold - self._raw0, self.raw_seen - hold), hold
        return out

    def _wave(self, raw: Optional[torch.Tensor], final: bool) -> torch.Tensor:
        ing = self.ing
        if ing.programmes is not None:
            return self._waves(raw, final)
        if raw is not None and raw.shape[-1]:
            if raw.dim() not in (1, 2) or raw.dtype not in (torch.float32, torch.int16) or (raw.dim() == 2 and not 1 <= raw.shape[0] <= 8):
                raise ValueError(f'raw wave: expected fp32 or int16 (n,) or (ch <= 8, n), got {raw.dtype} {tuple(raw.shape)}')
            x = raw.to(ing.dev, non_blocking=True)
            x = x[None] if x.dim() == 1 else x
            if self._passthrough(x):                                             # a mono fp32 wave at 16 kHz passes as it is
                self.raw_seen += int(x.shape[1])
                self.samples_out += int(x.shape[1])
                return x.reshape(-1)
            self._raw = x if self._raw is None else torch.cat([self._raw, x], 1)
            self.raw_seen += int(x.shape[1])
        if self._raw is None:
            return torch.empty(0, device=ing.dev, dtype=torch.float32)
        from . import ops
        c0, k0, k1, hold = resample_stream_plan(self.samples_out, self.raw_seen, ing.o, ing.width, ing.n, final)
        out = torch.empty(0, device=ing.dev, dtype=torch.float32)
        if k1 > k0:
            out = ops.resample_wave(self._raw[:, c0 - self._raw0:], ing.kernel, ing.o, ing.width, len_out=k1)[k0:]
            self.samples_out += k1 - k0
        self._raw, self._raw0 = self._raw[:, hold - self._raw0:], hold
        return out
