"""Mel post-processing on MI355X -- what the reference's scripts do right after the sampler (generate_sample.py:115-145,
inference_pipeline.py:382-396): ``denormalize_mel`` (utils/audio.py:17-19) -> ``exp`` -> ``torchaudio.transforms.InverseMelScale``
-> ``torchaudio.transforms.GriffinLim``.  The two transform classes keep torchaudio's constructor arguments and call
conventions so that the reference's scripts can swap the import; their arithmetic runs in libedtts_hip.so
(include/edtts.h: edtts_mel_to_spec, edtts_griffin_lim and their *_len twins).  The constant tables (mel filter bank and its
pseudo-inverse, Hann window, FFT twiddles) are built once on the host, like the schedule tables.

Ragged batches: ``lengths`` (int64 [B] frame counts of rows padded to a common T) gives row b bitwise what the
call on the row alone gives; ``smooth`` is the box filter of the reference's long-form tail (inference_pipeline.py:376-399) fused
into the inverse mel scale; ``MelVocoder.from_linear`` takes the list of stitched linear mels that
``InpaintSampler.generate_long_batch`` returns and vocodes all of them in one inverse-mel and one Griffin-Lim call.

PARITY UNPINNED: torchaudio is not available offline, so these ops are checked against the oracle's restatement of torchaudio's
published algorithm (the test suite's CPU oracle), not against outputs of the reference itself.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import native


def normalize_mel(mel: torch.Tensor):
    """utils/audio.py:10-14 (plain tensor algebra; statistics only, not on the hot path)."""
    mean = mel.mean(dim=1, keepdim=True)
    std = mel.std(dim=1, keepdim=True).clamp_min(1e-5)
    return (mel - mean) / std, mean, std


def denormalize_mel(mel_n: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """utils/audio.py:17-19."""
    return mel_n * std + mean


SMOOTH_MAX, SMOOTH_MAX_MELS = 9, 256  # csrc/edtts_melpost.h: kSmoothMax, kSmoothMaxMels


def check_smooth(smooth, n_mels: int) -> Tuple[int, int]:
    """smooth = (mel bins, frames) of the box filter -> (kh, kw); ValueError unless both are odd ints in [1, SMOOTH_MAX]."""
    try:
        kh, kw = smooth
    except (TypeError, ValueError):
        raise ValueError(f"smooth: expected (mel bins, frames), e.g. (5, 3), got {smooth!r}") from None
    for k in (kh, kw):
        if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k % 2 == 0 or k > SMOOTH_MAX:
            raise ValueError(f"smooth: the box filter's sides are odd ints in [1, {SMOOTH_MAX}], got {smooth!r}")
    if n_mels > SMOOTH_MAX_MELS:
        raise ValueError(f"smooth: built for n_mels <= {SMOOTH_MAX_MELS}, got {n_mels}")
    return kh, kw


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale="htk") -> [n_freqs, n_mels] (CPU, fp32)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


class InverseMelScale(torch.nn.Module):
    """torchaudio.transforms.InverseMelScale(n_stft, n_mels, sample_rate, f_min, f_max, norm=None, mel_scale="htk", driver="gelsd"):
    melspec [..., n_mels, T] -> relu(least-squares spectrogram) [..., n_stft, T]."""

    def __init__(self, n_stft: int, n_mels: int = 128, sample_rate: int = 16000, f_min: float = 0.0, f_max: Optional[float] = None,
                 norm: Optional[str] = None, mel_scale: str = "htk", driver: str = "gelsd"):
        super().__init__()
        if norm is not None or mel_scale != "htk" or driver != "gelsd":
            raise NotImplementedError("only norm=None, mel_scale='htk', driver='gelsd' (what the reference uses) are built")
        f_max = float(sample_rate // 2) if f_max is None else f_max
        fb = melscale_fbanks(n_stft, f_min, f_max, n_mels, sample_rate)
        self.n_stft, self.n_mels = n_stft, n_mels
        self.register_buffer("fb", fb)
        # minimum-norm least squares == multiplication by the pseudo-inverse (evaluated once, in fp64)
        self.register_buffer("pinv", torch.linalg.pinv(fb.t().double()).float().contiguous())
        # the index-error word of the calls with lengths (native.index_errors(self.idx_err) reads and clears it)
        self.register_buffer("idx_err", torch.zeros(1, dtype=torch.int32), persistent=False)

    @torch.no_grad()
    def forward(self, melspec: torch.Tensor, *, log_normalized: Optional[tuple] = None, lengths: Optional[torch.Tensor] = None,
                smooth: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """lengths (int64 [B] over the flattened leading dims, see native.lengths): row b equals the call on melspec[b, :, :lengths[b]]
        alone, bitwise, and its frames past lengths[b] are 0 (their input is never read).  smooth = (mel bins, frames), e.g. the
        reference's (5, 3): the inverse mel scale of F.avg_pool2d(melspec, smooth, stride=1, padding=(smooth[0] // 2, smooth[1] // 2)),
        a row's own end being the filter's edge; both odd, at most 9."""
        shape = melspec.shape
        x = melspec.reshape(-1, shape[-2], shape[-1]).transpose(1, 2).contiguous()  # [B, T, n_mels]: the kernels' frame-major layout
        return self._spec(x, None, None, lengths, smooth).reshape(shape[:-2] + (self.n_stft, shape[-1]))

    def _spec(self, mel_btm: torch.Tensor, mean, std, lengths=None, smooth=None) -> torch.Tensor:
        B, T, M = mel_btm.shape
        if M != self.n_mels:
            raise ValueError(f"expected {self.n_mels} mel bins, got {M}")
        if smooth is not None and mean is not None:
            raise ValueError("smooth: the box filter takes the linear mel spectrogram, not the normalised log-mel of from_normalized")
        box = check_smooth(smooth, M) if smooth is not None else None
        lens = native.lengths(lengths, B, T, mel_btm.device, "lengths")
        spec = native.mel_to_spec(mel_btm, mean, std, self.pinv, lens, box, self.idx_err)
        if lens is not None:
            native.check_indices(self.idx_err)
        return spec

    @torch.no_grad()
    def from_normalized(self, mel_n: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, *, lengths: Optional[torch.Tensor] = None,
                        smooth=None) -> torch.Tensor:
        """Fused generate_sample.py:115-144: denormalize_mel -> exp -> (transpose) -> inverse mel scale; mel_n [B, T, n_mels],
        mean / std [B, 1, n_mels] -> power spectrogram [B, n_stft, T].  lengths: as forward.  smooth is refused here: the box filter
        belongs to the linear mel."""
        B, T, M = mel_n.shape
        if smooth is not None:
            raise ValueError("smooth: the box filter takes the linear mel spectrogram, not the normalised log-mel of from_normalized")
        return self._spec(mel_n.contiguous(), mean.expand(B, 1, M).reshape(B, M).contiguous(), std.expand(B, 1, M).reshape(B, M).contiguous(),
                          lengths)


class GriffinLim(torch.nn.Module):
    """torchaudio.transforms.GriffinLim(n_fft, n_iter=32, win_length=None, hop_length=None, power=2.0, momentum=0.99, length=None,
    rand_init=True): specgram [..., n_fft // 2 + 1, T] -> waveform [..., hop * (T - 1)]."""

    def __init__(self, n_fft: int = 400, n_iter: int = 32, win_length: Optional[int] = None, hop_length: Optional[int] = None,
                 power: float = 2.0, momentum: float = 0.99, length: Optional[int] = None, rand_init: bool = True):
        super().__init__()
        win_length = n_fft if win_length is None else win_length
        if win_length != n_fft or length is not None or not rand_init:
            raise NotImplementedError("win_length == n_fft, length=None, rand_init=True (what the reference uses) are built")
        if not 0 <= momentum < 1:
            raise ValueError("momentum must be in [0, 1)")
        self.n_fft, self.n_iter, self.hop = n_fft, n_iter, (win_length // 2 if hop_length is None else hop_length)
        self.power, self.momentum = power, momentum
        self.register_buffer("window", torch.hann_window(win_length))
        q = torch.arange(n_fft // 2, dtype=torch.float64) * (-2.0 * math.pi / n_fft)
        self.register_buffer("twiddle", torch.stack([torch.cos(q), torch.sin(q)], dim=1).float().contiguous())
        # the index-error word of the calls with lengths (native.index_errors(self.idx_err) reads and clears it)
        self.register_buffer("idx_err", torch.zeros(1, dtype=torch.int32), persistent=False)

    @torch.no_grad()
    def forward(self, specgram: torch.Tensor, *, angles0: Optional[torch.Tensor] = None, seed: int = 0,
                lengths: Optional[torch.Tensor] = None, seeds=None):
        """Without lengths: the waveform [..., hop * (T - 1)].  With lengths (int64 [B] frame counts over the flattened leading dims,
        rows padded to T; see native.lengths): (wave [..., hop * (T - 1)], wave_lengths = hop * (lengths - 1)) -- row b is, bitwise in
        its first hop * (lengths[b] - 1) samples, this call on specgram[b:b+1, :, :lengths[b]] alone with seed = seeds[b] (or
        angles0[b:b+1, :, :lengths[b]]), and 0 behind them.  seeds: B ints or an int64 [B] tensor (native.seed_tensor); default: `seed`
        for every row.  A row with hop * (lengths[b] - 1) <= n_fft // 2 is a ValueError (CPU lengths), as the call on it alone."""
        shape = specgram.shape
        spec = specgram.reshape(-1, shape[-2], shape[-1]).to(torch.float32).contiguous()
        B, F, T = spec.shape
        if F != self.n_fft // 2 + 1:
            raise ValueError(f"expected {self.n_fft // 2 + 1} frequency bins, got {F}")
        if lengths is None and seeds is not None:
            raise ValueError("seeds: per-row seeds come with lengths (without lengths the batch draws from `seed`)")
        if lengths is not None:
            return self._forward_len(spec, shape, angles0, seed, lengths, seeds)
        a0 = None if angles0 is None else torch.view_as_real(angles0.reshape(B, F, T).to(torch.complex64)).contiguous()
        wave = native.griffin_lim(spec, self.n_fft, self.hop, self.window, self.twiddle, self.n_iter, self.momentum, self.power, a0, seed)
        return wave.reshape(shape[:-2] + (wave.shape[-1],))

    def _forward_len(self, spec, shape, angles0, seed, lengths, seeds):
        B, F, T = spec.shape
        if isinstance(lengths, torch.Tensor) and not lengths.is_cuda and lengths.dtype == torch.int64 and tuple(lengths.shape) == (B,) and B:
            short = int(lengths.min())
            if short >= 1 and self.hop * (short - 1) <= self.n_fft // 2:
                raise ValueError(f"lengths: a row of {short} frames gives {self.hop * (short - 1)} samples, not longer than the reflect "
                                 f"padding {self.n_fft // 2} (torch.stft raises too)")
        lens = native.lengths(lengths, B, T, spec.device, "lengths")
        sd = None
        if angles0 is None:
            sd = native.seed_tensor([seed] * B if seeds is None else seeds, B, spec.device)
        elif seeds is not None:
            native.seed_tensor(seeds, B, "cpu" if not isinstance(seeds, torch.Tensor) else seeds.device)  # shape check only: unused
        a0 = None if angles0 is None else torch.view_as_real(angles0.reshape(B, F, T).to(torch.complex64)).contiguous()
        wave = native.griffin_lim(spec, self.n_fft, self.hop, self.window, self.twiddle, self.n_iter, self.momentum, self.power, a0,
                                  t_len=lens, seeds=sd, idx_err=self.idx_err)
        native.check_indices(self.idx_err)
        return wave.reshape(shape[:-2] + (wave.shape[-1],)), (lens.clamp(1, T) - 1) * self.hop


class MelVocoder(torch.nn.Module):
    """generate_sample.py:115-145 in one object: normalised mel [B, T, n_mels] (+ the utterance's mean / std) -> waveform."""

    def __init__(self, cfg, n_iter: int = 32):
        super().__init__()
        self.inverse_mel = InverseMelScale(n_stft=cfg.n_fft // 2 + 1, n_mels=cfg.n_mels, sample_rate=cfg.sample_rate, f_min=cfg.f_min, f_max=cfg.f_max)
        self.griffin_lim = GriffinLim(n_fft=cfg.n_fft, n_iter=n_iter, win_length=cfg.win_length, hop_length=cfg.hop_length, power=2.0)

    @torch.no_grad()
    def forward(self, mel_n: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, *, angles0=None, seed: int = 0):
        spec = self.inverse_mel.from_normalized(mel_n, mean, std)
        return self.griffin_lim(spec, angles0=angles0, seed=seed)

    def pad_linear(self, mels: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        """The list of linear mels [n_mels, T_n] as one zero-padded batch [N, n_mels, max T_n] and the T_n (argument checks included)."""
        mels = list(mels)
        if not mels:
            raise ValueError("from_linear: an empty list of mels")
        n_mels, hop, n_fft = self.inverse_mel.n_mels, self.griffin_lim.hop, self.griffin_lim.n_fft
        for n, m in enumerate(mels):
            if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.shape[0] != n_mels:
                got = list(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__
                raise ValueError(f"from_linear: entry {n}: expected a linear mel [{n_mels}, T], got {got}")
            if hop * (m.shape[1] - 1) <= n_fft // 2:
                raise ValueError(f"from_linear: entry {n}: {m.shape[1]} frames give {hop * (m.shape[1] - 1)} samples, not longer than the "
                                 f"reflect padding {n_fft // 2} (torch.stft raises too)")
            if m.device != mels[0].device:
                raise ValueError(f"from_linear: entry {n} is on {m.device}, entry 0 on {mels[0].device}")
        frames = [int(m.shape[1]) for m in mels]
        batch = torch.zeros(len(mels), n_mels, max(frames), dtype=torch.float32, device=mels[0].device)
        for n, m in enumerate(mels):
            batch[n, :, :frames[n]] = m
        return batch, frames

    @torch.no_grad()
    def from_linear(self, mels: Sequence[torch.Tensor], *, smooth: Optional[Tuple[int, int]] = (5, 3), n_iter: Optional[int] = None,
                    seeds=None, angles0: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """The reference's long-form tail (inference_pipeline.py:376-399: avg_pool2d -> InverseMelScale -> GriffinLim) for a list of
        stitched linear mels [n_mels, T_n] of different lengths -- what InpaintSampler.generate_long_batch returns -- in one smoothed
        inverse-mel call and one ragged Griffin-Lim call: a list of waveforms [hop * (T_n - 1)] in the caller's order.  Entry n is
        bitwise from_linear([mels[n]], seeds=[seeds[n]]).  smooth: the box filter (mel bins, frames), None for none; n_iter overrides
        the constructor's (the reference runs 100 here, 32 in generate_sample.py); seeds: one int per entry (default 0 for each);
        angles0: per entry the complex initial phases [n_fft // 2 + 1, T_n] instead of library draws (parity runs)."""
        batch, frames = self.pad_linear(mels)
        N, dev = len(frames), batch.device
        if seeds is not None and not isinstance(seeds, torch.Tensor) and len(list(seeds)) != N:
            raise ValueError(f"seeds: expected {N} seeds (one per entry), got {len(list(seeds))}")
        a0 = None
        if angles0 is not None:
            angles0 = list(angles0)
            F = self.griffin_lim.n_fft // 2 + 1
            if len(angles0) != N or any(tuple(a.shape) != (F, t) for a, t in zip(angles0, frames)):
                raise ValueError(f"angles0: expected {N} tensors [{F}, T_n], one per entry")
            a0 = torch.zeros(N, F, max(frames), dtype=torch.complex64, device=dev)
            for n, a in enumerate(angles0):
                a0[n, :, :frames[n]] = a
        lens = torch.tensor(frames, dtype=torch.int64)
        lens = native.host_to_device(lens, dev) if dev.type == "cuda" else lens
        spec = self.inverse_mel(batch, lengths=lens, smooth=smooth)
        gl = self.griffin_lim
        keep, gl.n_iter = gl.n_iter, gl.n_iter if n_iter is None else int(n_iter)
        try:
            wave, _ = gl(spec, angles0=a0, lengths=lens, seeds=seeds)
        finally:
            gl.n_iter = keep
        hop = gl.hop
        return [wave[n, :hop * (frames[n] - 1)] for n in range(N)]
