"""GPU: the recording path - sf_track_decode against a float64 restatement of its recurrence, the segment feature bank against per-window tower launches,
the row-map windows against forward_clips and the CPU oracle, and the OffsetTracker API."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C21 = 21


# ----------------------------------------------------------------------------------------------------------------------------------------------
# the decode recurrence, restated in numpy (float64 unless told otherwise):
#   e[w, c] = l[w, c] - max_c l[w, .];  s_0 = e[0];  s_w[c] = max_p (s_{w-1}[p] - lam |p - c|) + e[w, c], lowest p on ties -> bp[w, c];
#   s_w -= max_c s_w[c];  end = argmax s_{W-1}, lowest index on ties;  backtrace through bp
# ----------------------------------------------------------------------------------------------------------------------------------------------
def _viterbi(logits: np.ndarray, lam: float, dt=np.float64):
    l = logits.astype(dt)
    lam = dt(lam)
    e = l - l.max(1, keepdims=True)
    W, C = e.shape
    d = np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(dt)        # d[p, c]
    s = e[0].copy()
    bp = np.zeros((W, C), np.int64)
    for w in range(1, W):
        cand = s[:, None] - lam * d
        bp[w] = cand.argmax(0)                                                   # first maximum = lowest p
        s = cand.max(0) + e[w]
        s = s - s.max()
    path = np.zeros(W, np.int64)
    path[-1] = s.argmax()
    for w in range(W - 1, 0, -1):
        path[w - 1] = bp[w, path[w]]
    return path


def _path_score(logits: np.ndarray, path: np.ndarray, lam: float) -> float:
    l = logits.astype(np.float64)
    e = l - l.max(1, keepdims=True)
    return float(e[np.arange(len(path)), path].sum() - lam * np.abs(np.diff(path.astype(np.int64))).sum())


def _best_score(logits: np.ndarray, lam: float) -> float:
    """The optimum of the objective in float64, without the renormalisation (a per-step constant, irrelevant to the maximum's argument but not to its value)."""
    l = logits.astype(np.float64)
    e = l - l.max(1, keepdims=True)
    C = e.shape[1]
    d = np.abs(np.arange(C)[:, None] - np.arange(C)[None, :]).astype(np.float64)
    s = e[0].copy()
    for w in range(1, e.shape[0]):
        s = (s[:, None] - lam * d).max(0) + e[w]
    return float(s.max())


def _softmax64(logits: np.ndarray) -> np.ndarray:
    l = logits.astype(np.float64)
    p = np.exp(l - l.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


def _decode(gpu, logits_np: np.ndarray, lam: float, ldl=None):
    from synchformer_amd import ops
    W, C = logits_np.shape
    if ldl is None:
        x = torch.from_numpy(logits_np.astype(np.float32)).to(gpu)
    else:                                                                        # a strided view: columns beyond C hold a value that would win every argmax
        buf = torch.full((W, ldl), 1e30, device=gpu, dtype=torch.float32)
        buf[:, :C] = torch.from_numpy(logits_np.astype(np.float32)).to(gpu)
        x = buf[:, :C]
    out = ops.track_decode(x, lam)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.int32, torch.float32] and all(t.shape == (W,) for t in out)
    return [t.cpu().numpy() for t in out]


def _check_exact(gpu, x: np.ndarray, lam: float, ldl=None):
    W = x.shape[0]
    cls_raw, conf_raw, cls_path, conf_path = _decode(gpu, x, lam, ldl)
    ref = _viterbi(x, lam)
    assert np.array_equal(cls_raw, x.argmax(1)), 'cls_raw'                        # numpy's argmax: first maximum
    assert np.array_equal(cls_path, ref), (lam, W, np.flatnonzero(cls_path != ref)[:8])
    p = _softmax64(x)
    err_raw = np.abs(conf_raw - p[np.arange(W), cls_raw]).max()
    err_path = np.abs(conf_path - p[np.arange(W), cls_path]).max()
    assert err_raw <= 2e-6 and err_path <= 2e-6, (err_raw, err_path)             # 21 terms, fp32 exp and sum
    if lam == 0:
        assert np.array_equal(cls_path, cls_raw)
    return cls_raw, cls_path


@pytest.mark.parametrize('W', [1, 2, 3, 64, 65, 1000])
@pytest.mark.parametrize('lam', [0.0, 0.5, 2.0, 64.0])
def test_decode_exact(gpu, lam, W):
    """Integer logits in [-8, 8], dyadic lam: every operation of the recurrence is exact in fp32 (scores are multiples of 0.5 bounded by 16 + 20 lam after the
    per-step renormalisation), so classes and path must equal the float64 restatement exactly, ties included; nothing is left to a tolerance.
    lam = 0 gives the argmax path.  lam = 64 gives a constant path where the recurrence itself does: it holds for these inputs up to W = 65 (the float64
    restatement agrees), and provably whenever lam >= 16 (W - 1).  At W = 1000 with independent uniform logits the OPTIMUM switches class (the difference of two
    classes' partial sums is a random walk with steps up to +-16: its excursions pass 64 within a few hundred windows), so that case is compared with the
    restatement like every other and the constant-path property at W = 1000 is checked on test_decode_strong_cost_gives_constant_path's input, where it is provable."""
    rng = np.random.default_rng(1000 * W + int(2 * lam))
    x = rng.integers(-8, 9, (W, C21)).astype(np.float64)
    cls_raw, cls_path = _check_exact(gpu, x, lam)
    if lam == 64.0 and W <= 65:
        assert (cls_path == cls_path[0]).all()


@pytest.mark.parametrize('W', [2, 65, 1000])
def test_decode_strong_cost_gives_constant_path(gpu, W):
    """lam = 64 must give a constant path.  Class 7 wins every even window by 8, class 12 every odd window by 8, all other classes lie 8 below the loser: the argmax
    alternates, while any path that leaves a class pays >= 64 and a run of r windows in the other class gains at most 8 (ceil(r / 2) - floor(r / 2)) <= 8 over staying:
    the optimum is constant (class 7: it wins window 0 and ties or leads in total; lowest index on ties)."""
    x = np.full((W, C21), -8.0)
    x[0::2, 7], x[1::2, 7] = 8.0, 0.0
    x[0::2, 12], x[1::2, 12] = 0.0, 8.0
    cls_raw, cls_path = _check_exact(gpu, x, 64.0)
    assert np.array_equal(cls_raw, np.where(np.arange(W) % 2 == 0, 7, 12))
    assert (cls_path == 7).all()


def test_decode_strided_and_two_classes(gpu):
    rng = np.random.default_rng(77)
    x = rng.integers(-8, 9, (130, C21)).astype(np.float64)
    _check_exact(gpu, x, 0.5, ldl=37)                                            # ldl > C: the columns beyond C must not be read
    for lam in (0.0, 0.5, 2.0, 64.0):
        x2 = rng.integers(-8, 9, (257, 2)).astype(np.float64)                    # C = 2, more than one block of the row kernels
        _check_exact(gpu, x2, lam)
    x64 = rng.integers(-8, 9, (66, 64)).astype(np.float64)                       # C = 64: every lane owns a class
    _check_exact(gpu, x64, 2.0)


@pytest.mark.parametrize('lam', [0.25, 1.0, 3.0])
def test_decode_real_valued(gpu, lam):
    """A ramp of the true class 5 -> 15 over 200 windows, N(0, 1) logits with +1.5 on the true class.  Real-valued scores round, so the returned path is scored in
    float64 and must lie within 2 W 3 2^-24 (max |e| + lam C) of the float64 optimum: three roundings per step of the renormalised recurrence."""
    W = 200
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((W, C21))
    true = np.round(np.linspace(5, 15, W)).astype(np.int64)
    x[np.arange(W), true] += 1.5
    x = x.astype(np.float32)
    cls_raw, conf_raw, cls_path, conf_path = _decode(gpu, x, lam)
    assert np.array_equal(cls_raw, x.argmax(1))
    e = x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True)
    bound = 2 * W * 3 * 2.0 ** -24 * (np.abs(e).max() + lam * C21)
    got, best = _path_score(x, cls_path, lam), _best_score(x, lam)
    print(f'lam {lam}: path score {got:.6f}, float64 optimum {best:.6f}, bound {bound:.2e}; path differs from argmax in {(cls_path != cls_raw).sum()} of {W} windows, '
          f'from the truth in {(cls_path != true).sum()} (argmax: {(cls_raw != true).sum()})')
    assert best - got <= bound and got <= best + 1e-9, (got, best, bound)
    p = _softmax64(x)
    assert np.abs(conf_path - p[np.arange(W), cls_path]).max() <= 2e-6 and np.abs(conf_raw - p[np.arange(W), cls_raw]).max() <= 2e-6


def test_decode_non_finite_logits_stay_in_range(gpu):
    """One row of NaN and one row of +inf: any classes may come out, but every class written lies in [0, C) - the backtrace never reads out of range."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, C21)).astype(np.float32)
    x[11, :] = np.nan
    x[23, :] = np.inf
    cls_raw, conf_raw, cls_path, conf_path = _decode(gpu, x, 1.0)
    for c in (cls_raw, cls_path):
        assert c.min() >= 0 and c.max() < C21, c
    assert np.array_equal(cls_raw[:11], x[:11].argmax(1))                        # rows before the first non-finite one are untouched in the raw read-out


# ----------------------------------------------------------------------------------------------------------------------------------------------
# the bank and the windows
# ----------------------------------------------------------------------------------------------------------------------------------------------
T_REC, N_REC, N_SEG = 144, 92160, 17


@pytest.fixture(scope='module')
def rec(gpu):
    """One engine (gain-1 synthetic weights, seg_chunk = 5), one 17-segment recording, its bank and the per-window references - computed once, read-only."""
    from synchformer_amd import synth
    from synchformer_amd.engine import SynchformerEngine
    from synchformer_amd.frontend import MelFrontend
    sd = synth.make_state_dict(1337)
    eng = SynchformerEngine(sd, gpu, seg_chunk=5)
    mel = MelFrontend(gpu)
    g = torch.Generator().manual_seed(99)
    frames = torch.randint(0, 256, (T_REC, 3, 224, 224), generator=g, dtype=torch.uint8)
    wave = synth.make_wave(1, 1, 99, n=N_REC).reshape(N_REC)
    fd, wd = frames.to(gpu), wave.to(gpu)
    vbank, abank = eng.extract_recording(fd, wd, mel)                            # chunks of 5, 5, 5, 2 segments
    clip_logits = {w: eng.forward_clips(fd[None, 8 * w:8 * w + 120], wd[None, 5120 * w:5120 * w + 76800], mel)[0].clone() for w in range(4)}
    torch.cuda.synchronize()
    return dict(sd=sd, eng=eng, mel=mel, frames=frames, wave=wave, fd=fd, wd=wd, vbank=vbank, abank=abank, clip_logits=clip_logits)


def test_bank_is_independent_of_chunking_and_input_placement(gpu, rec):
    eng, mel = rec['eng'], rec['mel']
    assert rec['vbank'].shape == (N_SEG, 8, 768) and rec['abank'].shape == (N_SEG, 6, 768) and rec['vbank'].dtype == rec['abank'].dtype == torch.float32
    vh, ah = eng.extract_recording(rec['frames'], rec['wave'], mel)              # the recording in (unpinned) host memory: uploaded chunk by chunk
    assert torch.equal(vh, rec['vbank']) and torch.equal(ah, rec['abank'])
    vp, ap = eng.extract_recording(rec['frames'].pin_memory(), rec['wave'].pin_memory(), mel, seg_chunk=4)      # pinned; 4, 4, 4, 4, 1
    assert torch.equal(vp, rec['vbank']) and torch.equal(ap, rec['abank'])
    v1, a1 = eng.extract_recording(rec['fd'], rec['wd'], mel, seg_chunk=1)       # one segment at a time
    assert torch.equal(v1, rec['vbank']) and torch.equal(a1, rec['abank'])
    assert eng.seg_chunk == 5


def test_audio_bank_equals_per_window_tower(gpu, rec):
    eng, mel = rec['eng'], rec['mel']
    for w in range(4):
        ref = eng.extract_afeats(mel.segments(rec['wd'][None, 5120 * w:5120 * w + 76800], 0, 5120, 14, 10240))[0]
        d = (rec['abank'][w:w + 14] - ref).abs().max().item()
        print(f'window {w}: max |abank - per-window audio tower| {d:.3e}')
        assert torch.equal(rec['abank'][w:w + 14], ref), (w, d)


def test_visual_bank_equals_per_window_tower(gpu, rec):
    """vbank[w:w+14] is bit-equal to extract_vfeats_clips on frames[8w:8w+120], for every w.  The engine's seg_chunk = 5 bounds both sides: the bank runs 5, 5, 5, 2
    segments, a 14-segment clip 5, 5, 4 - launches of the un-fused tower schedule, where a segment's output does not depend on its place in the launch
    (test_chunking_invariance).  (A 14-segment launch of the FUSED schedule would not be comparable bit for bit: sf_gemm_res_ln768 rotates its k-loop by
    workgroup, so two such launches differ by 6e-3 on the segments they share - extract_vfeats_clips honours seg_chunk inside a clip for that reason too.)"""
    eng = rec['eng']
    refs = [eng.extract_vfeats_clips(rec['fd'][None, 8 * w:8 * w + 120], 0, 8, 14)[0].clone() for w in range(4)]
    ds = [(rec['vbank'][w:w + 14] - refs[w]).abs().max().item() for w in range(4)]
    print(f'max |vbank - per-window visual tower| per window {ds}; feature std {refs[0].std().item():.3f}')
    for w in range(4):
        assert torch.equal(rec['vbank'][w:w + 14], refs[w]), (w, ds[w])


@pytest.mark.parametrize('hop, W', [(1, 4), (2, 2)])
def test_windows_equal_forward_clips(gpu, rec, hop, W):
    """track(...).logits[w] against forward_clips on the explicit slice frames[8 hop w : 8 hop w + 120]: every launch treats rows independently of M at these
    sizes, so the two are bit-equal on the MI355X (measured maximum difference 0).  The windows differ among themselves (a tracker that returned one window W
    times would fail), and the sync stage alone is bit-equal too: a row-map window equals sync_transformer on the sliced bank, whatever win_chunk."""
    from synchformer_amd.track import OffsetTracker
    tracker = OffsetTracker(rec['eng'], rec['mel'], hop_segments=hop)
    tr = tracker.track(rec['fd'], rec['wd'])
    assert tr.logits.shape == (W, C21) and tr.n_segments == N_SEG
    ref = torch.stack([rec['clip_logits'][hop * w] for w in range(W)])
    err = (tr.logits - ref).abs().max().item()
    spread = (ref - ref.mean(0, keepdim=True)).abs().max().item()
    print(f'hop {hop}: max |track logits - forward_clips| {err:.3e}, windows differ by up to {spread:.3e}, bit-equal: {torch.equal(tr.logits, ref)}')
    assert torch.equal(tr.logits, ref), err
    assert spread > 5 * err and spread > 1e-4, (spread, err)                    # (1e-4: far above one fp32 ulp of a logit - the windows really differ)
    # the windows of a pass are independent: 3 + 1 windows per pass give the logits of one pass of 4
    small = tracker.track_features(rec['vbank'], rec['abank'], win_chunk=3).logits
    assert torch.equal(small, tracker.track_features(rec['vbank'], rec['abank'], win_chunk=256).logits) and torch.equal(small, tr.logits)
    for w in range(W):
        lo = hop * w
        one = rec['eng'].sync_transformer(rec['vbank'][None, lo:lo + 14], rec['abank'][None, lo:lo + 14])[0]
        assert torch.equal(tr.logits[w], one), (w, (tr.logits[w] - one).abs().max().item())


def test_sync_windows_match_oracle(gpu, rec):
    from oracle import synchformer_cpu as O
    from synchformer_amd.track import OffsetTracker
    g = torch.Generator().manual_seed(11)
    vb, ab = torch.randn(N_SEG, 8, 768, generator=g), torch.randn(N_SEG, 6, 768, generator=g)
    sd = rec['sd']
    for hop, W in ((1, 4), (2, 2)):
        got = OffsetTracker(rec['eng'], rec['mel'], hop_segments=hop).track_features(vb.to(gpu), ab.to(gpu)).logits.cpu()
        with torch.no_grad():
            pv, pa = O._lin(vb, sd, 'vproj'), O._lin(ab, sd, 'aproj')
            v = torch.stack([pv[hop * w:hop * w + 14].reshape(-1, 768) for w in range(W)])
            a = torch.stack([pa[hop * w:hop * w + 14].reshape(-1, 768) for w in range(W)])
            ref = O.global_transformer(v, a, sd)
        err = (got - ref).abs().max().item()
        spread = (ref - ref.mean(0, keepdim=True)).abs().max().item()
        print(f'hop {hop}: max |sync_windows - oracle| {err:.3e}, windows differ by up to {spread:.3e}')
        assert got.shape == ref.shape == (W, C21) and err < 1.5e-2, err


def test_offset_track_end_to_end(gpu, rec):
    from synchformer_amd.postprocess import class_grid
    from synchformer_amd.track import OffsetTrack, OffsetTracker
    eng, mel = rec['eng'], rec['mel']
    tracker = OffsetTracker(eng, mel, hop_segments=1, lam=0.5)
    tr = tracker.track_features(rec['vbank'], rec['abank'])
    assert isinstance(tr, OffsetTrack) and tr.n_segments == N_SEG
    W = 4
    want = dict(t_sec=torch.float32, cls_raw=torch.int32, conf_raw=torch.float32, cls_path=torch.int32, conf_path=torch.float32, offset_sec_raw=torch.float32,
                offset_sec_path=torch.float32)
    for name, dt in want.items():
        t = getattr(tr, name)
        assert t.shape == (W,) and t.dtype == dt, (name, t.shape, t.dtype)
    assert tr.logits.shape == (W, C21) and tr.logits.dtype == torch.float32
    assert torch.equal(tr.t_sec.cpu(), torch.tensor([(8 * w + 60) / 25 for w in range(W)], dtype=torch.float64).float())
    grid = class_grid(-2, 2, 21)
    assert torch.equal(tr.offset_sec_raw.cpu(), grid[tr.cls_raw.cpu().long()]) and torch.equal(tr.offset_sec_path.cpu(), grid[tr.cls_path.cpu().long()])
    assert torch.equal(tr.cls_raw.cpu(), tr.logits.argmax(1).cpu().int())
    x = tr.logits.cpu().numpy()
    e = x.astype(np.float64) - x.astype(np.float64).max(1, keepdims=True)
    assert _best_score(x, 0.5) - _path_score(x, tr.cls_path.cpu().numpy(), 0.5) <= 2 * W * 3 * 2.0 ** -24 * (np.abs(e).max() + 0.5 * C21)
    p = torch.softmax(tr.logits.double(), 1).cpu()
    assert (tr.conf_raw.cpu() - p[torch.arange(W), tr.cls_raw.cpu().long()]).abs().max() <= 2e-6
    # below one window: 119 frames hold 13 segments
    with pytest.raises(ValueError, match='13 segments'):
        tracker.track(rec['fd'][:119], rec['wd'])
    with pytest.raises(ValueError):
        tracker.track(rec['fd'], rec['wd'][:76799])
    with pytest.raises(ValueError, match='classes'):
        OffsetTracker(eng, mel, grid=torch.tensor([0.0, 1.0]))                 # a 2-way grid on the 21-way engine
    with pytest.raises(ValueError):
        OffsetTracker(eng, mel, lam=-1.0)
