"""Audio front end on MI355X -- the two torchaudio ops the reference calls at every entry point:
``torchaudio.functional.resample`` (LJSpeech's 22.05 kHz -> CFG.sample_rate; generate_sample.py:75-80, data/collate.py:34-37,
inference_pipeline.py:206-207) and ``torchaudio.transforms.MelSpectrogram`` followed by ``log(clamp(., 1e-5))`` and
``normalize_mel`` (the (mean, std) that denormalise every generated mel, generate_sample.py:97-116; the per-chunk statistics of the
long-form loop, inference_pipeline.py:349-355; the training target, data/collate.py:58-60).

The classes keep torchaudio's constructor arguments and call conventions so that the reference's scripts can swap the import; their
arithmetic runs in libedtts_hip.so (include/edtts.h: edtts_melspec, edtts_mel_segment_stats, edtts_logmel_stats, edtts_resample).
The constant tables (Hann window, FFT twiddles, the mel filter bank's non-zero ranges, the polyphase sinc table) are built once on
the host, like the Griffin-Lim tables.

Sinc table precision: ``resample`` (the functional) builds it in fp32 arithmetic, as torchaudio's functional does in the
waveform's dtype; ``Resample`` (the transform) builds it in fp64 and casts, as torchaudio's transform does with ``dtype=None``
(or in the ``dtype`` it is given).

PARITY UNPINNED: torchaudio is not available offline, so these ops are checked against the test suite's fp64 restatement of
torchaudio's published algorithm (cross-checked against transformers' numpy spectrogram and scipy's upfirdn), not against outputs of
torchaudio itself.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import native
from .native import EDTTS_MEL_LOG, EDTTS_MEL_POWER
from .melpost import melscale_fbanks

N_FFT = 1024


# ---------------------------------------------------------------------------------------------------- host tables
def mel_filter_ranges(fb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fb [n_freqs, n_mels] -> (desc int32 [n_mels, 3] = (first bin, bin count, offset), packed weights fp32): each filter's
    contiguous non-zero bin range (an HTK triangle), its weights in ascending bin order."""
    desc, weights, off = [], [], 0
    for m in range(fb.shape[1]):
        nz = torch.nonzero(fb[:, m]).flatten()
        if nz.numel() == 0:
            desc.append((0, 0, off))
            continue
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        desc.append((lo, hi - lo, off))
        weights.append(fb[lo:hi, m])
        off += hi - lo
    w = torch.cat(weights) if weights else torch.zeros(1)
    return torch.tensor(desc, dtype=torch.int32), w.to(torch.float32).contiguous()


def fft_twiddle(n_fft: int = N_FFT) -> torch.Tensor:
    """[n_fft / 2, 2] = exp(-2 pi i q / n_fft), evaluated in fp64 (the Griffin-Lim table)."""
    q = torch.arange(n_fft // 2, dtype=torch.float64) * (-2.0 * math.pi / n_fft)
    return torch.stack([torch.cos(q), torch.sin(q)], dim=1).float().contiguous()


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                         dtype: Optional[torch.dtype] = torch.float32) -> Tuple[torch.Tensor, int]:
    """torchaudio.functional's _get_sinc_resample_kernel (sinc_interp_hann) for orig / new already divided by their gcd ->
    (h [new, 2 width + orig] fp32, width): h[p][j] = (base / orig) sinc(pi u) cos^2(pi u / (2 lpw)),
    u = clamp(((j - width) / orig - p / new) base, -lpw, lpw), base = min(orig, new) rolloff.  dtype is the arithmetic: fp32 as the
    functional (the waveform's dtype), None = fp64 then cast, as the transform."""
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    base_freq = min(orig_freq, new_freq) * rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base_freq)
    idx_dtype = dtype if dtype is not None else torch.float64
    idx = torch.arange(-width, width + orig_freq, dtype=idx_dtype)[None, None] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=dtype)[:, None, None] / new_freq + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / orig_freq
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels.reshape(new_freq, -1).to(torch.float32).contiguous(), width


def polyphase_table(h: torch.Tensor) -> torch.Tensor:
    """h [new, K] -> the kernel's B-fragment layout [ceil(K / 4), round_up(new, 16), 4], zero-padded (include/edtts.h)."""
    new, K = h.shape
    Kp, Np = -(-K // 4) * 4, -(-new // 16) * 16
    hp = torch.zeros(Np, Kp, dtype=torch.float32)
    hp[:new, :K] = h
    return hp.reshape(Np, Kp // 4, 4).permute(1, 0, 2).contiguous()


def resampled_length(n: int, orig_freq: int, new_freq: int) -> int:
    """torchaudio's output length ceil(new * n / orig) (orig / new reduced or not), in exact integer arithmetic."""
    return -(-int(n) * int(new_freq) // int(orig_freq))


def frame_count(n: int, hop: int) -> int:
    """Frames of a centred STFT of n samples: n // hop + 1."""
    return int(n) // int(hop) + 1


# ---------------------------------------------------------------------------------------------------- resampling
_TABLES = {}


def _resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, dtype, device):
    if resampling_method == "sinc_interp_kaiser":
        raise NotImplementedError("resampling_method='sinc_interp_kaiser' is not built: only 'sinc_interp_hann' (what the reference uses)")
    if resampling_method != "sinc_interp_hann":
        raise ValueError(f"Invalid resampling method: {resampling_method}")
    if not (int(orig_freq) == orig_freq and int(new_freq) == new_freq):
        raise Exception("Frequencies must be of integer type to ensure quality resampling computation. ")
    gcd = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // gcd, int(new_freq) // gcd
    key = (o, n, lowpass_filter_width, float(rolloff), dtype, str(device))
    if key not in _TABLES:
        h, width = sinc_resample_kernel(o, n, lowpass_filter_width, rolloff, dtype)
        _TABLES[key] = (o, n, width, h.shape[1], polyphase_table(h).to(device))
    return _TABLES[key]


def _resample(waveform, plan, lengths):
    o, n, width, taps, table = plan
    shape = waveform.shape
    x = waveform.reshape(-1, shape[-1]).to(torch.float32).contiguous()
    B, L = x.shape
    if B == 0 or L == 0:
        raise ValueError("resample: empty waveform")
    L_out = resampled_length(L, o, n)
    lens = native.lengths(lengths, B, L, x.device, "lengths")
    y = native.resample(x, lens, o, n, width, taps, table, L_out).reshape(shape[:-1] + (L_out,))
    if lengths is None:
        return y
    return y, (lens.clamp(1, L) * n + (o - 1)) // o


@torch.no_grad()
def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None, *, lengths: Optional[torch.Tensor] = None):
    """torchaudio.functional.resample: waveform [..., L] -> [..., ceil(new L / orig)] (sinc table in fp32 arithmetic).  ``lengths``
    (int64 [B] over the flattened leading dims): row b equals the call on waveform[b, :lengths[b]] alone, its outputs past
    ceil(new lengths[b] / orig) are 0, and (output, output lengths) is returned."""
    if orig_freq <= 0.0 or new_freq <= 0.0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if orig_freq == new_freq:
        return waveform if lengths is None else (waveform, lengths)
    plan = _resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, torch.float32, waveform.device)
    return _resample(waveform, plan, lengths)


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta, dtype): the sinc
    table is built once, in fp64 and cast (dtype None, torchaudio's default) or in ``dtype``."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = "sinc_interp_hann",
                 lowpass_filter_width: int = 6, rolloff: float = 0.99, beta: Optional[float] = None, *,
                 dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.orig_freq, self.new_freq = orig_freq, new_freq
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta, self.dtype = (
            resampling_method, lowpass_filter_width, rolloff, beta, dtype)
        if orig_freq != new_freq:
            _resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, dtype, "cpu")  # argument checks

    @torch.no_grad()
    def forward(self, waveform: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        if self.orig_freq == self.new_freq:
            return waveform if lengths is None else (waveform, lengths)
        plan = _resample_plan(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method, self.dtype,
                              waveform.device)
        return _resample(waveform, plan, lengths)


# ---------------------------------------------------------------------------------------------------- mel analysis
class MelSpectrogram(torch.nn.Module):
    """torchaudio.transforms.MelSpectrogram with its signature and defaults.  Built: n_fft = win_length = 1024, pad 0, periodic Hann
    window, power 2.0 or 1.0, normalized False, center True, pad_mode "reflect", onesided, norm None, mel_scale "htk" (what the
    reference uses: generate_sample.py, data/collate.py, inference_pipeline.py).  forward(wav [..., L]) -> [..., n_mels, L // hop + 1].

    Additions: ``log_mel`` (log(max(mel, 1e-5)) frame-major, what normalize_mel consumes), ``stats`` (normalize_mel's mean / std of
    it) and ``segment_stats`` (the statistics of many slices of the batch, each as if it were its own waveform, in one launch)."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, win_length: Optional[int] = None, hop_length: Optional[int] = None,
                 f_min: float = 0.0, f_max: Optional[float] = None, pad: int = 0, n_mels: int = 128, window_fn=torch.hann_window,
                 power: float = 2.0, normalized: bool = False, wkwargs: Optional[dict] = None, center: bool = True,
                 pad_mode: str = "reflect", onesided: Optional[bool] = None, norm: Optional[str] = None, mel_scale: str = "htk"):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        built = (n_fft == N_FFT and win_length == N_FFT and pad == 0 and window_fn is torch.hann_window and not wkwargs and
                 power in (1.0, 2.0) and not normalized and center and pad_mode == "reflect" and onesided in (None, True) and norm is None
                 and mel_scale == "htk" and 1 <= n_mels <= 128 and 1 <= hop_length <= n_fft)
        if not built:
            raise NotImplementedError("MelSpectrogram: only n_fft = win_length = 1024, pad=0, window_fn=torch.hann_window (periodic), "
                                      "power 2.0 or 1.0, normalized=False, center=True, pad_mode='reflect', onesided, norm=None, "
                                      "mel_scale='htk', 1 <= n_mels <= 128, 1 <= hop_length <= n_fft are built")
        self.sample_rate, self.n_fft, self.win_length, self.hop_length = sample_rate, n_fft, win_length, hop_length
        self.f_min, self.f_max, self.n_mels, self.power = f_min, f_max, n_mels, power
        f_max = float(sample_rate // 2) if f_max is None else f_max
        self.register_buffer("fb", melscale_fbanks(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate))
        desc, w = mel_filter_ranges(self.fb)
        self.register_buffer("fb_desc", desc)
        self.register_buffer("fb_weights", w)
        self.register_buffer("window", torch.hann_window(win_length))
        self.register_buffer("twiddle", fft_twiddle(n_fft))

    def frames(self, n_samples: int) -> int:
        return frame_count(n_samples, self.hop_length)

    def _rows(self, wav: torch.Tensor, lengths) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        x = wav.reshape(-1, wav.shape[-1]) if wav.dim() != 2 else wav
        x = x.to(torch.float32).contiguous()
        B, L = x.shape
        if L <= self.n_fft // 2:
            raise RuntimeError(f"MelSpectrogram: a signal of {L} samples is not longer than the reflect padding {self.n_fft // 2} "
                               "(torch.stft raises too)")
        if lengths is not None and isinstance(lengths, torch.Tensor) and not lengths.is_cuda and lengths.numel() == B and B:
            if int(lengths.min()) <= self.n_fft // 2:
                raise ValueError(f"lengths: {int(lengths.min())} samples are not longer than the reflect padding {self.n_fft // 2}")
        return x, native.lengths(lengths, B, L, x.device, "lengths")

    def _tables(self):
        return self.window, self.twiddle, self.fb_desc, self.fb_weights

    def _melspec(self, x, lens, mode):
        return native.melspec(x, lens, self.n_fft, self.hop_length, self._tables(), self.n_mels, int(self.power), mode)

    @torch.no_grad()
    def forward(self, waveform: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[..., L] -> mel [..., n_mels, L // hop + 1] (power or magnitude).  lengths: int64 per flattened row, as log_mel."""
        x, lens = self._rows(waveform, lengths)
        out = self._melspec(x, lens, EDTTS_MEL_POWER)
        return out.reshape(waveform.shape[:-1] + out.shape[-2:])

    @torch.no_grad()
    def log_mel(self, wav: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """log(clamp(mel, 1e-5)).transpose(1, 2): wav [B, L] -> [B, L // hop + 1, n_mels] (generate_sample.py:97-100,
        data/collate.py:58-60).  lengths: int64 [B]; row b then equals the call on wav[b:b+1, :lengths[b]] alone, bitwise, in its
        first lengths[b] // hop + 1 frames, and its later frames are 0."""
        if self.power != 2.0:
            raise NotImplementedError("log_mel / stats are built for power=2.0 (what the reference uses)")
        x, lens = self._rows(wav, lengths)
        return self._melspec(x, lens, EDTTS_MEL_LOG)

    @torch.no_grad()
    def stats(self, wav: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """normalize_mel(log_mel(wav))[1:]: (mean, std), each [B, 1, n_mels] -- unbiased std clamped at 1e-5, over each row's own
        frames; what MelVocoder takes (generate_sample.py:97-116)."""
        if self.power != 2.0:
            raise NotImplementedError("log_mel / stats are built for power=2.0 (what the reference uses)")
        x, lens = self._rows(wav, lengths)
        lm = self._melspec(x, lens, EDTTS_MEL_LOG)
        return native.logmel_stats(lm, x.shape[1], lens, self.hop_length)

    @torch.no_grad()
    def segment_stats(self, wav: torch.Tensor, rows, starts, ends, lengths: Optional[torch.Tensor] = None):
        """(mean, std), each [n_seg, 1, n_mels]: segment i gives exactly stats(wav[rows[i]:rows[i]+1, starts[i]:min(ends[i], len)]) --
        reflect padding at the segment's own ends, (e - s) // hop + 1 frames, one frame -> NaN std.  All segments in one launch.
        rows / starts / ends: sequences of ints, or int64 tensors (device tensors are used as they are: graph-capturable)."""
        if self.power != 2.0:
            raise NotImplementedError("log_mel / stats are built for power=2.0 (what the reference uses)")
        x, lens = self._rows(wav, lengths)
        B, L = x.shape
        if all(isinstance(v, torch.Tensor) and v.is_cuda for v in (rows, starts, ends)):
            seg = torch.stack([rows.to(torch.int64), starts.to(torch.int64), ends.to(torch.int64)], dim=1).contiguous()
        else:
            rows, starts, ends = ([int(v) for v in (s.tolist() if isinstance(s, torch.Tensor) else s)] for s in (rows, starts, ends))
            if not (len(rows) == len(starts) == len(ends)) or not rows:
                raise ValueError("rows, starts and ends: one entry per segment, at least one segment")
            for i, (r, s, e) in enumerate(zip(rows, starts, ends)):
                if not 0 <= r < B:
                    raise ValueError(f"segment {i}: row {r} outside [0, {B})")
                if s < 0 or min(e, L) - s <= self.n_fft // 2:
                    raise ValueError(f"segment {i}: [{s}, {e}) of a {L}-sample row is not longer than the reflect padding {self.n_fft // 2}")
            seg = torch.tensor(list(zip(rows, starts, ends)), dtype=torch.int64).to(x.device)
        return native.mel_segment_stats(x, lens, seg, self.n_fft, self.hop_length, self._tables(), self.n_mels)


def chunk_segments(totals: Sequence[int], chunk_samples: int, overlap_samples: int) -> List[List[Tuple[int, int]]]:
    """Per utterance the [start, end) sample slices of the reference's sliding window (inference_pipeline.py:221-225, 298-300, 354):
    hop = chunk - overlap, n = ceil((total - overlap) / hop) chunks (InpaintSampler.chunk_plan), chunk i = [i hop, i hop + chunk) cut
    at the utterance's end."""
    from .longform import InpaintSampler
    out = []
    for total in totals:
        n, c, h = InpaintSampler.chunk_plan(0, 0, 0, 1, chunk_samples, overlap_samples, int(total))
        out.append([(i * h, min(i * h + c, int(total))) for i in range(n)])
    return out


@torch.no_grad()
def chunk_stats_from_audio(wavs: Sequence[torch.Tensor], chunk_samples: int, overlap_samples: int, mel: MelSpectrogram):
    """Per utterance the list of per-chunk (mean [1, 1, n_mels], std [1, 1, n_mels]) that InpaintSampler.generate_long_batch(...,
    chunk_stats=...) takes: normalize_mel of the log-mel of wav[:, start:end] of every chunk (inference_pipeline.py:354-355), all chunks
    of all utterances in one launch.  wavs: 1-D (or [1, L]) fp32 device tensors of the utterances' samples."""
    rows = [w.reshape(-1) for w in wavs]
    totals = [int(r.numel()) for r in rows]
    plans = chunk_segments(totals, chunk_samples, overlap_samples)
    batch = torch.zeros(len(rows), max(totals), dtype=torch.float32, device=rows[0].device)
    for i, r in enumerate(rows):
        batch[i, :totals[i]] = r
    seg = [(n, s, e) for n, p in enumerate(plans) for s, e in p]
    for n, s, e in seg:
        if e - s <= mel.n_fft // 2:
            raise ValueError(f"utterance {n}: chunk [{s}, {e}) is not longer than the reflect padding {mel.n_fft // 2} "
                             "(torchaudio raises for it too)")
    mean, std = mel.segment_stats(batch, [s[0] for s in seg], [s[1] for s in seg], [s[2] for s in seg])
    out, k = [], 0
    for p in plans:
        out.append([(mean[k + i:k + i + 1], std[k + i:k + i + 1]) for i in range(len(p))])
        k += len(p)
    return out
