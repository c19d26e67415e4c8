"""Host tests of the audio front end (edge_diffusion_tts_amd/audio.py): the fp64 restatements the GPU parity tests use, cross-checked
against independent implementations present offline (transformers' numpy spectrogram, scipy's upfirdn); the product's host tables;
the output-length and frame-count arithmetic; the API's errors and the new C symbols.  No GPU.

The restatements (ref_*) are torchaudio's published algorithm written on torch ops: MelSpectrogram = torch.stft(center, reflect,
periodic Hann) -> |.|^2 -> @ melscale_fbanks; resample = the sinc_interp_hann polyphase table applied by conv1d at stride orig."""
import math

import numpy as np
import pytest
import torch

from edge_diffusion_tts_amd import CFG, InpaintSampler, MelSpectrogram, Resample, native, resample
from edge_diffusion_tts_amd import audio
from edge_diffusion_tts_amd.melpost import melscale_fbanks

RATES = [22050, 24000, 44100, 48000, 8000]


# ------------------------------------------------------------------------------------------------ restatements (also used on the GPU)
def ref_fb(n_mels=80, sr=16000, f_min=0.0, f_max=8000.0):
    return melscale_fbanks(513, f_min, f_max, n_mels, sr)


def ref_mel(wav, hop=160, dtype=torch.float64, fb=None, power=2.0):
    """wav [B, L] (CPU) -> power (or, power = 1.0, magnitude) mel [B, n_mels, T] computed in `dtype` (fp32 = what torchaudio itself
    computes); fb: the filter bank [513, n_mels], default ref_fb()."""
    fb = ref_fb() if fb is None else fb
    x = wav.to(dtype)
    spec = torch.stft(x, 1024, hop, 1024, window=torch.hann_window(1024, dtype=dtype), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    p = spec.abs() ** 2 if power == 2.0 else spec.abs() ** power
    return torch.matmul(p.transpose(-1, -2), fb.to(dtype)).transpose(-1, -2)


def ref_log_mel(wav, hop=160, dtype=torch.float64, *, fb=None, power=2.0):
    return torch.log(torch.clamp(ref_mel(wav, hop, dtype, fb, power), min=1e-5)).transpose(1, 2)


def ref_stats(log_mel):
    """normalize_mel (utils/audio.py:10-14)"""
    return log_mel.mean(dim=1, keepdim=True), log_mel.std(dim=1, keepdim=True).clamp_min(1e-5)


def ref_sinc_table(orig, new, lpw=6, rolloff=0.99, dtype=torch.float64):
    """h [new, 2 w + orig] from the formula, in `dtype` arithmetic; orig / new reduced by their gcd."""
    base = min(orig, new) * rolloff
    w = math.ceil(lpw * orig / base)
    j = torch.arange(2 * w + orig, dtype=dtype)
    p = torch.arange(new, dtype=dtype)[:, None]
    u = (((j - w) / orig)[None, :] - p / new) * base
    u = u.clamp(-lpw, lpw)
    win = torch.cos(u * math.pi / lpw / 2) ** 2
    s = torch.where(u == 0, torch.ones((), dtype=dtype), torch.sin(math.pi * u) / (math.pi * u))
    return s * win * (base / orig), w


def ref_resample(x, orig_freq, new_freq, dtype=torch.float64, lpw=6, rolloff=0.99):
    """x [B, L] (CPU) -> [B, ceil(new L / orig)]: torchaudio's _apply_sinc_resample_kernel in `dtype`."""
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    h, w = ref_sinc_table(o, n, lpw, rolloff, dtype)
    B, L = x.shape
    xp = torch.nn.functional.pad(x.to(dtype), (w, w + o))
    y = torch.nn.functional.conv1d(xp[:, None], h[:, None, :], stride=o)
    y = y.transpose(1, 2).reshape(B, -1)
    return y[:, :-(-n * L // o)]


def signals(B, L, seed, kind="mix"):
    """Seeded synthetic test audio: chirps, tones, noise and near-silence (down to the 1e-5 clamp)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 16000
    out = []
    for b in range(B):
        k = (b + seed) % 4 if kind == "mix" else {"chirp": 0, "tone": 1, "noise": 2, "quiet": 3}[kind]
        if k == 0:
            f0, f1 = 100 + 50 * b, 7000
            x = 0.5 * torch.sin(2 * math.pi * (f0 * t + (f1 - f0) * t ** 2 / (2 * t[-1].clamp_min(1e-3))))
        elif k == 1:
            x = 0.3 * torch.sin(2 * math.pi * (220 + 37 * b) * t) + 0.1 * torch.sin(2 * math.pi * 3100 * t)
        elif k == 2:
            x = 0.2 * torch.randn(L, generator=g, dtype=torch.float64)
        else:
            x = 1e-5 * torch.randn(L, generator=g, dtype=torch.float64)
        out.append(x)
    return torch.stack(out).float()


# ------------------------------------------------------------------------------------------------ restatement cross-checks
def test_mel_restatement_matches_transformers_spectrogram():
    au = pytest.importorskip("transformers.audio_utils")
    wav = signals(3, 16000 + 77, 1)
    fb = ref_fb().double()
    ours = ref_mel(wav, 160, torch.float64)
    for b in range(3):
        theirs = au.spectrogram(wav[b].double().numpy(), torch.hann_window(1024, dtype=torch.float64).numpy(), frame_length=1024,
                                hop_length=160, fft_length=1024, power=2.0, center=True, pad_mode="reflect", onesided=True,
                                mel_filters=fb.numpy(), mel_floor=0.0, dtype=np.float64)
        theirs = torch.from_numpy(theirs)
        assert theirs.shape == ours[b].shape
        # transformers keeps the complex STFT in complex64 whatever `dtype` says (audio_utils.spectrogram): agreement to fp32 rounding
        assert float((theirs - ours[b]).abs().max()) <= 1e-6 * float(theirs.abs().max())


def test_transformers_bank_is_the_product_bank():
    au = pytest.importorskip("transformers.audio_utils")
    theirs = au.mel_filter_bank(num_frequency_bins=513, num_mel_filters=80, min_frequency=0.0, max_frequency=8000.0, sampling_rate=16000,
                                norm=None, mel_scale="htk")
    assert theirs.shape == (513, 80)
    assert float(np.abs(theirs - ref_fb().double().numpy()).max()) <= 1e-5  # torchaudio's bank is built in fp32, transformers' in fp64


@pytest.mark.parametrize("orig", RATES)
def test_resample_restatement_matches_upfirdn(orig):
    sig = pytest.importorskip("scipy.signal")
    new = 16000
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    x = signals(1, 3 * orig // 10 + 13, 3, "noise").double()[0]
    y = ref_resample(x[None], orig, new)[0]
    # the same filter on the fine grid of rate o n: hfull[k] = f(-k / (o n)), |k| <= R; upfirdn(h, x, up=n, down=o)[i + s] = y[i]
    base, lpw = min(o, n) * 0.99, 6
    R = int(math.floor(lpw / base * o * n))
    s = -(-R // o)
    k = torch.arange(-s * o, R + 1, dtype=torch.float64)
    u = (-k / (o * n) * base).clamp(-lpw, lpw)
    f = torch.where(u == 0, torch.ones((), dtype=torch.float64), torch.sin(math.pi * u) / (math.pi * u))
    f = f * torch.cos(u * math.pi / lpw / 2) ** 2 * (base / o)
    y2 = torch.from_numpy(sig.upfirdn(f.numpy(), x.numpy(), up=n, down=o))
    assert y2.shape[0] >= s + y.shape[0]
    assert float((y2[s:s + y.shape[0]] - y).abs().max()) <= 1e-12


def test_resampled_sine_is_the_sine():
    L = 22050
    t = torch.arange(L, dtype=torch.float64) / 22050
    x = torch.sin(2 * math.pi * 1000 * t)
    y = ref_resample(x[None], 22050, 16000)[0]
    assert y.shape[0] == 16000
    want = torch.sin(2 * math.pi * 1000 * torch.arange(16000, dtype=torch.float64) / 16000)
    assert float((y - want)[400:-400].abs().max()) <= 1e-3


# ------------------------------------------------------------------------------------------------ product tables
def test_product_tables_equal_the_restatement():
    mel = MelSpectrogram(16000, n_fft=1024, win_length=1024, hop_length=160, f_min=0, f_max=8000, n_mels=80)
    assert torch.equal(mel.window, torch.hann_window(1024))
    assert torch.equal(mel.fb, ref_fb())
    # the filter ranges rebuild the bank exactly, each range is contiguous, the bank is sparse as stated
    fb = torch.zeros(513, 80)
    for m, (lo, cnt, off) in enumerate(mel.fb_desc.tolist()):
        fb[lo:lo + cnt, m] = mel.fb_weights[off:off + cnt]
        assert cnt == 0 or (2 <= cnt <= 40)
    assert torch.equal(fb, mel.fb)
    assert int(mel.fb_desc[:, 1].sum()) == int((mel.fb != 0).sum())
    q = torch.arange(512, dtype=torch.float64) * (-2 * math.pi / 1024)
    assert torch.allclose(mel.twiddle.double(), torch.stack([q.cos(), q.sin()], 1), atol=1e-7)
    for orig in RATES:
        g = math.gcd(orig, 16000)
        o, n = orig // g, 16000 // g
        h32, w = audio.sinc_resample_kernel(o, n, 6, 0.99, torch.float32)
        h64, _ = audio.sinc_resample_kernel(o, n, 6, 0.99, None)
        ref, wr = ref_sinc_table(o, n)
        assert w == wr and h32.shape == ref.shape == (n, 2 * w + o)
        # fp32 arithmetic (the functional): sin / cos of arguments up to 6 pi in fp32; fp64 (the transform): torchaudio still forms
        # the phase term arange(0, -new, -1) / new in the default fp32 dtype before adding the fp64 index
        assert float((h32.double() - ref).abs().max()) <= 3e-5
        assert float((h64.double() - ref).abs().max()) <= 1e-5
        tab = audio.polyphase_table(h32)
        Kp, Np = -(-(2 * w + o) // 4) * 4, -(-n // 16) * 16
        assert tab.shape == (Kp // 4, Np, 4)
        back = tab.permute(1, 0, 2).reshape(Np, Kp)
        assert torch.equal(back[:n, :2 * w + o], h32) and not back[n:].any() and not back[:, 2 * w + o:].any()


def test_the_issue_tap_counts():
    taps = {}
    for orig in RATES:
        g = math.gcd(orig, 16000)
        h, w = audio.sinc_resample_kernel(orig // g, 16000 // g)
        taps[orig] = (orig // g, 16000 // g, h.shape[1])
    assert taps == {22050: (441, 320, 459), 24000: (3, 2, 23), 44100: (441, 160, 475), 48000: (3, 1, 41), 8000: (1, 2, 15)}


# (orig, new) -> (taps, p-tiles per group PT, groups, grid.y, dynamic LDS bytes) of k_resample: the paths test_audio_gpu.py's
# test_resample_launch_geometries is meant to reach
GEOMETRY = {
    (16000, 22050): (334, 1, 28, 7, 42304),   # upsampling: 28 one-tile groups, 7 grid rows
    (16000, 44100): (174, 1, 28, 7, 21184),
    (44100, 40000): (455, 5, 5, 2, 58272),    # PT = 5 with a second grid row, 57 KB of LDS
    (11025, 16000): (455, 5, 8, 2, 58272),
    (16000, 48000): (15, 1, 1, 1, 192),       # K padded from 15 to 16
    (32000, 48000): (16, 1, 1, 1, 320),       # K = 16: no remainder
    (48000, 44100): (174, 5, 2, 1, 21184),
    (22050, 16000): (459, 5, 4, 1, 58288),    # the rates of test_resample_parity
    (44100, 16000): (475, 5, 2, 1, 58352),
    (24000, 16000): (23, 1, 1, 1, 480),
    (48000, 16000): (41, 1, 1, 1, 560),
    (8000, 16000): (15, 1, 1, 1, 192),
}


def resample_geometry(orig, new):
    """edtts_resample's launch arithmetic (csrc/edtts_audio.h) on the product's sinc table."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    h, w = audio.sinc_resample_kernel(o, n)
    taps = h.shape[1]
    assert taps == 2 * w + o
    Kp, Np = (taps + 3) & ~3, (n + 15) & ~15
    tiles = Np // 16
    PT = 5 if tiles % 5 == 0 else 1
    groups = tiles // PT
    return taps, PT, groups, (groups + 3) // 4, (16 * 2 * o + Kp) * 4


def test_resample_launch_geometries():
    import os
    src = open(os.path.join(os.path.dirname(audio.__file__), "..", "csrc", "edtts_audio.h")).read()
    # the lines resample_geometry restates: a retune of the tile grouping has to come through here
    for line in ("constexpr int kRsMB = 2;", "const int Kp = (taps + 3) & ~3, Np = (new_freq + 15) & ~15;",
                 "const int tiles = Np / 16, PT = tiles % 5 == 0 ? 5 : 1, n_groups = tiles / PT;",
                 "const size_t lds = (size_t)(16 * kRsMB * orig + Kp) * sizeof(float);", "(unsigned)((n_groups + 3) / 4)"):
        assert line in src, line
    for rates, want in GEOMETRY.items():
        assert resample_geometry(*rates) == want, rates
        assert want[4] <= 64 * 1024


def test_length_arithmetic():
    for orig in RATES:
        for L in (1, 2, 440, 441, 442, 22050, 110251, 220500, 1234567):
            want = int(math.ceil(16000 * L / orig))
            assert audio.resampled_length(L, orig, 16000) == want
            assert ref_resample(torch.zeros(1, L), orig, 16000).shape[1] == want if L < 300000 else True
    for L in (513, 1000, 16000, 16159, 16160, 16161, 160000):
        T = torch.stft(torch.zeros(L), 1024, 160, window=torch.hann_window(1024), center=True, return_complex=True).shape[1]
        assert audio.frame_count(L, 160) == T == L // 160 + 1


# ------------------------------------------------------------------------------------------------ API
def test_unsupported_arguments_raise():
    ok = dict(sample_rate=16000, n_fft=1024, win_length=1024, hop_length=160, f_min=0, f_max=8000, n_mels=80)
    MelSpectrogram(**ok)
    MelSpectrogram(**{**ok, "power": 1.0})
    for bad in ({"n_fft": 400, "win_length": None}, {"win_length": 800}, {"pad": 4}, {"window_fn": torch.hamming_window},
                {"power": 3.0}, {"power": None}, {"normalized": True}, {"center": False}, {"pad_mode": "constant"}, {"onesided": False},
                {"norm": "slaney"}, {"mel_scale": "slaney"}, {"wkwargs": {"periodic": False}}, {"n_mels": 129}):
        with pytest.raises(NotImplementedError, match="built"):
            MelSpectrogram(**{**ok, **bad})
    with pytest.raises(NotImplementedError):
        MelSpectrogram()  # torchaudio's default n_fft = 400
    with pytest.raises(NotImplementedError, match="kaiser"):
        resample(torch.zeros(1, 100), 22050, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(NotImplementedError, match="kaiser"):
        Resample(22050, 16000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError):
        resample(torch.zeros(1, 100), 22050, 16000, resampling_method="linear")
    with pytest.raises(ValueError):
        resample(torch.zeros(1, 100), 0, 16000)
    with pytest.raises(ValueError):
        resample(torch.zeros(1, 100), 22050, 16000, lowpass_filter_width=0)
    x = torch.zeros(2, 100)
    assert resample(x, 16000, 16000) is x  # orig == new returns the input
    assert Resample(16000, 16000)(x) is x
    mel = MelSpectrogram(**ok)
    with pytest.raises(RuntimeError, match="reflect padding"):
        mel.log_mel(torch.zeros(1, 512))


def test_new_symbols_are_declared_exported_and_bound():
    L = native.lib()
    for sym in ("edtts_melspec", "edtts_mel_segment_stats", "edtts_logmel_stats", "edtts_resample"):
        assert hasattr(L, sym), sym
    assert L.edtts_version() == 400


def test_library_rejects_bad_sizes():
    L = native.lib()
    p = 16  # any non-NULL pointer: the checks run before anything is launched
    with pytest.raises(native.EdttsError, match="n_fft=512"):
        L.edtts_melspec(p, 1, 4000, None, 512, 160, p, p, p, p, 80, 2, 1, p, None)
    with pytest.raises(native.EdttsError, match="power=3"):
        L.edtts_melspec(p, 1, 4000, None, 1024, 160, p, p, p, p, 80, 3, 1, p, None)
    with pytest.raises(native.EdttsError, match="reflect padding"):
        L.edtts_melspec(p, 1, 512, None, 1024, 160, p, p, p, p, 80, 2, 1, p, None)
    with pytest.raises(native.EdttsError, match="NULL"):
        L.edtts_mel_segment_stats(p, 1, 4000, None, None, 1, 1024, 160, p, p, p, p, 80, p, p, None)
    with pytest.raises(native.EdttsError, match="taps"):
        L.edtts_resample(p, 1, 4000, None, 441, 320, 9, 458, p, 2903, p, None)
    with pytest.raises(native.EdttsError, match="LDS"):
        L.edtts_resample(p, 1, 4000, None, 2003, 1000, 13, 2029, p, 1998, p, None)


def test_chunk_segments_follow_the_reference_arithmetic():
    chunk, ov = 32000, 8000
    totals = [8001, 32000, 32001, 56000, 56001, 100000, 123457]
    segs = audio.chunk_segments(totals, chunk, ov)
    for total, sg in zip(totals, segs):
        hop = chunk - ov
        n = int(np.ceil((total - ov) / hop))  # inference_pipeline.py:225
        assert len(sg) == max(1, n)
        assert sg == [(i * hop, min(i * hop + chunk, total)) for i in range(len(sg))]  # wav[:, start:end] (:300, :354)
        n_plan = InpaintSampler.chunk_plan(0, 0, 0, 1, chunk, ov, total)[0]
        assert n_plan == len(sg)
    assert InpaintSampler.chunk_stats_from_audio is not None
