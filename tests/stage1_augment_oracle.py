"""CPU restatement of the Stage-1 train-time augmentations (sf_stage1_video_augment, sf_stage1_audio_augment) in plain torch / numpy, with a
`dtype` switch: torch.float32 mirrors the reference op by op (torchvision 0.15's tensor path on uint8 - _blend, rgb_to_grayscale, adjust_hue
with _rgb2hsv / _hsv2rgb, resize through F.interpolate - and torchaudio's Vol / lowpass_biquad), torch.float64 is the yardstick.  Also the
inputs the GPU tests run on, so that the CPU self-check can prove their bounds reachable by the reference arithmetic alone.  A helper module:
tests/test_stage1_augment_cpu.py and tests/test_stage1_augment_gpu.py import it; nothing in the package does."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from synchformer_amd import augment as A

N_PIX = 224 * 224


# ---- video ----------------------------------------------------------------------------------------------------------------------------------------
def crop(frames: torch.Tensor, y0: int, x0: int, side: int, dtype) -> torch.Tensor:
    """frames uint8 (T, 3, H, W) -> uint8 (T, 3, 224, 224): the 224 crop, or the 192 crop through Resize(224, antialias=None) - bilinear,
    align_corners=False, in `dtype`, torch.round (half to even) back to uint8."""
    x = frames[..., y0:y0 + side, x0:x0 + side]
    if side == 224:
        return x.clone()
    return F.interpolate(x.to(dtype), size=(224, 224), mode='bilinear', align_corners=False).round().to(torch.uint8)


def gray(x: torch.Tensor, dtype) -> torch.Tensor:
    """rgb_to_grayscale: (0.2989 r + 0.587 g + 0.114 b).to(uint8), (T, 3, h, w) -> (T, 1, h, w)."""
    r, g, b = (x[:, i:i + 1].to(dtype) for i in range(3))
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(torch.uint8)


def blend(a: torch.Tensor, b, ratio: float, dtype) -> torch.Tensor:
    """_blend: (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(uint8); ratio a Python float, so fp32 sees float32(ratio), float32(1 - ratio)."""
    b = b.to(dtype) if torch.is_tensor(b) else b
    return (ratio * a.to(dtype) + (1.0 - ratio) * b).clamp(0, 255).to(torch.uint8)


def brightness(x, ratio, dtype):
    return blend(x, torch.zeros_like(x), ratio, dtype)


def saturation(x, ratio, dtype):
    return blend(x, gray(x, dtype), ratio, dtype)


def contrast(x, ratio, dtype):
    """mean over (C, H, W) of the gray image PER FRAME (x is (T, 3, h, w), torchvision reduces dims (-3, -2, -1))."""
    g = gray(x, dtype).to(dtype)
    mean = g.sum(dim=(-3, -2, -1), keepdim=True) / g[0].numel()
    return blend(x, mean, ratio, dtype)


def _rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc, minc = torch.max(img, dim=-3).values, torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / cr_divisor, (maxc - g) / cr_divisor, (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - (s * f))), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6).view(-1, 1, 1)
    a1, a2, a3 = torch.stack((v, q, p, p, t, v), dim=-3), torch.stack((t, v, v, q, p, p), dim=-3), torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum('...ijk, ...xijk -> ...xjk', mask.to(dtype=img.dtype), a4)


def hue(x, hue_factor: float, dtype):
    """adjust_hue: x / 255 -> HSV -> h = (h + f) % 1.0 -> RGB -> .mul(255 + 1.0 - 1e-3).to(uint8)."""
    img = _rgb2hsv(x.to(dtype).div(255))
    h, s, v = img.unbind(dim=-3)
    h = (h + hue_factor) % 1.0
    return _hsv2rgb(torch.stack((h, s, v), dim=-3)).mul(255 + 1.0 - 1e-3).to(torch.uint8)


def colour_row(row: torch.Tensor):
    """(jitter, order, (brightness, contrast, saturation ratios as Python floats), hue, gray, flip) of a segment-table row."""
    f = A.bits_f32(row[A.S1_BRIGHT:A.S1_HUE + 1].contiguous())
    return bool(row[A.S1_JITTER]), [int(o) for o in row[A.S1_OP0:A.S1_OP0 + 4]], (float(f[0]), float(f[2]), float(f[4])), float(f[6]), \
        bool(row[A.S1_GRAY]), bool(row[A.S1_FLIP])


def video_segment(x: torch.Tensor, row: torch.Tensor, dtype) -> torch.Tensor:
    """Cropped frames uint8 (T, 3, 224, 224) + a segment-table row -> the augmented frames: ColorJitter in the row's order, RandomGrayscale, flip."""
    jitter, order, ratios, hf, to_gray, flip = colour_row(row)
    if jitter:
        for op in order:
            if op == A.S1_OP_BRIGHTNESS:
                x = brightness(x, ratios[0], dtype)
            elif op == A.S1_OP_CONTRAST:
                x = contrast(x, ratios[1], dtype)
            elif op == A.S1_OP_SATURATION:
                x = saturation(x, ratios[2], dtype)
            elif op == A.S1_OP_HUE:
                x = hue(x, hf, dtype)
    if to_gray:
        x = gray(x, dtype).expand(-1, 3, -1, -1)
    return x.flip(-1) if flip else x


def video_augment(frames: torch.Tensor, clip_table: torch.Tensor, seg_table: torch.Tensor, n_seg: int, v_stride: int, dtype, seg_frames=None) -> torch.Tensor:
    """frames uint8 (B, T, 3, H, W) + host tables -> uint8 (B * n_seg, len(seg_frames), 3, 224, 224); seg_frames: which of a segment's 16 frames
    (all by default - the frames of a segment do not depend on each other)."""
    seg_frames = list(range(16)) if seg_frames is None else list(seg_frames)
    out = []
    for n in range(frames.shape[0] * n_seg):
        b, s = divmod(n, n_seg)
        f0, y0, x0, side = (int(v) for v in clip_table[b, :4])
        idx = torch.tensor([f0 + s * v_stride + f for f in seg_frames])
        out.append(video_segment(crop(frames[b, idx], y0, x0, side, dtype), seg_table[n], dtype))
    return torch.stack(out)


def clamp_tables(clip_table, seg_table, n_seg, v_stride, a_stride, a_size, T, n_samples, H, W):
    """What the kernels make of out-of-range rows: every clip entry clamped into the clip, a side other than 192 taken as 224."""
    c = clip_table.clone()
    c[:, 3] = torch.where(c[:, 3] == 192, 192, 224)
    c[:, 0] = c[:, 0].clamp(0, T - ((n_seg - 1) * v_stride + 16))
    c[:, 1] = torch.minimum(c[:, 1].clamp(min=0), H - c[:, 3])
    c[:, 2] = torch.minimum(c[:, 2].clamp(min=0), W - c[:, 3])
    c[:, 4] = c[:, 4].clamp(0, n_samples - ((n_seg - 1) * a_stride + a_size))
    return c, seg_table.clone()


# ---- audio ----------------------------------------------------------------------------------------------------------------------------------------
def audio_gather(wave: torch.Tensor, clip_table: torch.Tensor, n_seg: int, a_stride: int, a_size: int) -> torch.Tensor:
    return torch.stack([wave[n // n_seg, int(clip_table[n // n_seg, 4]) + (n % n_seg) * a_stride:][:a_size] for n in range(wave.shape[0] * n_seg)])


def volume(x: torch.Tensor) -> torch.Tensor:
    return (x * 2.0).clamp(-1, 1)                       # Vol(gain=2.0, gain_type='amplitude')


def lowpass(x: np.ndarray, coeffs, dtype) -> np.ndarray:
    """lowpass_biquad -> lfilter(clamp=True) on rows of x, zero initial state, every operation in `dtype` (np.float32 | np.float64); the
    coefficients are the double ones divided by a0, cast to float32 first (what the device receives)."""
    b0, b1, b2, a1, a2 = (dtype(np.float32(c)) for c in coeffs)
    x = x.astype(dtype)
    y = np.zeros_like(x)
    z = np.zeros(x.shape[0], dtype=dtype)
    x1, x2, y1, y2 = z, z, z, z
    for i in range(x.shape[1]):
        x0 = x[:, i]
        y0 = (b0 * x0 + b1 * x1 + b2 * x2) - (a1 * y1 + a2 * y2)
        y[:, i] = y0
        x2, x1, y2, y1 = x1, x0, y1, y0
    return np.clip(y, -1, 1)


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------------------
T, H, W, N_SAMPLES = 40, 232, 250, 40000


@functools.lru_cache(None)
def clips() -> torch.Tensor:
    """2 clips of 40 frames, 232 x 250 (W no multiple of 4), content that differs per frame: noise under a per-frame brightness, with quantised,
    tied-channel and gray bands (the inputs on which the fp32 / fp64 disagreement was measured)."""
    g = torch.Generator().manual_seed(20)
    x = torch.randint(0, 256, (2, T, 3, H, W), generator=g, dtype=torch.uint8)
    level = (0.15 + 0.85 * ((torch.arange(T) * 7) % 16) / 15).view(1, T, 1, 1, 1)
    x = (x.float() * level).to(torch.uint8)
    x[:, :, :, 40:80] = x[:, :, :, 40:80] // 32 * 32                 # quantised
    x[:, :, 1, 100:130] = x[:, :, 0, 100:130]                        # r == g
    x[:, :, :, 150:170] = x[:, :, :1, 150:170]                       # gray
    x[:, :, :, 200:210, :60] = 255
    x[:, :, :, 200:210, 60:120] = 0
    return x


@functools.lru_cache(None)
def waves() -> torch.Tensor:
    g = torch.Generator().manual_seed(21)
    t = torch.arange(N_SAMPLES) / 16000
    return (0.4 * torch.randn(2, N_SAMPLES, generator=g) + 0.3 * torch.sin(2 * np.pi * 60 * t)).float()


def seg_rows(n: int, **cols) -> torch.Tensor:
    """n neutral segment rows (no jitter, identity order, factors 1, hue 0), then the given columns: jitter / gray / flip / audio / seed (lists),
    order (n x 4), bright / contrast / satur (ratios), hue."""
    t = torch.zeros(n, A.S1_SEG_COLS, dtype=torch.int32)
    t[:, A.S1_OP0:A.S1_OP0 + 4] = torch.arange(4, dtype=torch.int32)
    one = dict(bright=A.S1_BRIGHT, contrast=A.S1_CONTRAST, satur=A.S1_SATUR)
    for k, col in one.items():
        r32, q32 = A.blend_pair(np.asarray(cols.get(k, [1.0] * n), dtype=np.float32))
        t[:, col], t[:, col + 1] = A.f32_bits(r32), A.f32_bits(q32)
    t[:, A.S1_HUE] = A.f32_bits(np.asarray(cols.get('hue', [0.0] * n), dtype=np.float32))
    for k, col in dict(jitter=A.S1_JITTER, gray=A.S1_GRAY, flip=A.S1_FLIP, audio=A.S1_AUDIO, seed=A.S1_SEED).items():
        if k in cols:
            t[:, col] = torch.tensor(cols[k], dtype=torch.int32)
    if 'order' in cols:
        t[:, A.S1_OP0:A.S1_OP0 + 4] = torch.tensor(cols['order'], dtype=torch.int32)
    return t


def clip_rows(rows) -> torch.Tensor:
    return torch.tensor(rows, dtype=torch.int32).view(len(rows), A.S1_CLIP_COLS)


# 2 clips x 2 segments of stride 16: an odd x0 at the top edge, and the far corner of the last frames (40 - 32 = 8, 232 - 224 = 8, 250 - 224 = 26)
CROP_ROWS = [[0, 0, 13, 224, 3], [8, 8, 26, 224, N_SAMPLES - 20480]]
UPSCALE_ROWS = [[0, 0, 7, 192, 0], [8, 40, 58, 192, 0]]          # the far corner of the 192 crop: 232 - 192 = 40, 250 - 192 = 58


def hue_case():
    return clip_rows(CROP_ROWS), seg_rows(4, jitter=[1] * 4, order=[[3, 0, 1, 2]] * 4, hue=[-0.2, -0.05, 0.1, 0.2]), 2, 16


def upscale_case():
    return clip_rows(UPSCALE_ROWS), seg_rows(4), 2, 16


ORDER_FRAMES = (0, 5, 10, 15)        # the frames of a segment the 24-order case is checked on (frames are independent of each other)


def orders_case():
    """24 segments (2 clips x 12 of stride 2), one op order each, random factors, mixed with gray, flip and the 192 crop (clip 1)."""
    import itertools
    g = torch.Generator().manual_seed(22)
    u = torch.rand(24, 4, generator=g)
    return clip_rows([[0, 3, 13, 224, 0], [2, 40, 57, 192, 0]]), \
        seg_rows(24, jitter=[1] * 24, order=list(itertools.permutations(range(4))), bright=(0.2 + 1.6 * u[:, 0]).tolist(),
                 contrast=(0.2 + 1.6 * u[:, 1]).tolist(), satur=(0.2 + 1.6 * u[:, 2]).tolist(), hue=(-0.2 + 0.4 * u[:, 3]).tolist(),
                 gray=[int(i % 5 == 4) for i in range(24)], flip=[i % 2 for i in range(24)]), 12, 2


@functools.lru_cache(None)
def reference(case: str, dtype_name: str) -> torch.Tensor:
    """The oracle's output for one of the cases above, computed once per process and shared by the tests (treat as read-only)."""
    clip_table, seg_table, n_seg, v_stride = dict(hue=hue_case, upscale=upscale_case, orders=orders_case)[case]()
    return video_augment(clips(), clip_table, seg_table, n_seg, v_stride, getattr(torch, dtype_name), ORDER_FRAMES if case == 'orders' else None)


def compare(a: torch.Tensor, b: torch.Tensor):
    """(largest difference in levels, share of differing pixels) of two uint8 tensors."""
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    return int(d.max()), float((d != 0).float().mean())
