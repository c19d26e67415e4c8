"""Long-form in-painting sampler -- the sampling core of /root/reference/inference_pipeline.py:97-196,296-367 on MI355X.

The reference keeps ``inpaint_student_sample`` and ``inpaint_teacher_refine`` as closures inside its pipeline script; here they
are methods of :class:`InpaintSampler` with the same arguments and arithmetic (v-prediction decoder on the ``sem_features``
context with a constant step index, q_sample of the previous chunk's tail forced onto the first ``overlap_len`` frames at every
step, optional classifier-free guidance against an all-zero context), each running as ONE C-ABI call
(include/edtts.h: edtts_sample_inpaint): context K/V built once per call (twice with guidance), the blend is a tiny elementwise
kernel, guidance combine + x0 / eps / next-x update are fused into the last transformer layer.  ``generate_long`` is the
reference's chunk loop (:296-367) as written: per-chunk de-normalisation, exp, cross-fade of LINEAR mels with the trapezoid
window, division by the summed weights (sequential: every chunk is conditioned on the tail of the previous one).
``generate_long_batch`` runs that loop for many utterances in lockstep: chunk i of every utterance that has one is refined in ONE
batched call (per-utterance semantic lengths and seeds), and each utterance's result is bitwise its ``generate_long`` alone.
``inpaint_dpm_refine`` is the teacher refinement with DPM-Solver++'s multistep update (schedule.py: DPMSolverPP) in place of the
first-order step -- the sampler the reference builds next to its pipeline and never calls -- as ONE C-ABI call
(edtts_sample_inpaint_multistep_len); ``generate_long(_batch)(..., solver="dpmpp")`` refines every chunk with it.
All three samplers take ``keep=``, a per-frame mask of the known frames in place of the known prefix (the reference's rule does not
depend on where they sit; edtts_sample_inpaint_mask_len, edtts_sample_inpaint_multistep_mask_len), and ``edit`` re-synthesises
stretches of an utterance with everything around them kept.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import native
from .schedule import DiffusionSchedule, DPMSolverPP

SOLVERS = ("ddim", "dpmpp")


def linspace_times(t_start: int, n: int) -> List[int]:
    """torch.linspace(t_start, 0, n + 1).long()[:-1] (inference_pipeline.py:101-102,165-166)."""
    return torch.linspace(t_start, 0, n + 1).long()[:-1].tolist()


def strictly_decreasing_times(times: Sequence[int]) -> List[int]:
    """DPMSolverPP.get_time_steps maps points equally spaced in log-SNR onto table rows.  Near the end of the table the log-SNR falls
    so fast that several points land on one row (t_start = 999, 15 steps: 999, 999, 999, 998, 998, 997, ...), and a step between two
    equal times has no log-SNR distance: the reference's own coefficients divide 0 by 0 there.  Each time is therefore capped at one
    below its predecessor (999, 998, 997, 996, 995, 994, ...): the same number of steps, every one with a distance.  A list that
    already decreases strictly (t_start = 500; the reference's own max_t = 950 at up to 16 steps) is returned as it is.  ValueError
    when the table has fewer rows below t_start than steps (the times end at 1)."""
    out = []
    for t in times:
        t = int(t) if not out else min(int(t), out[-1] - 1)
        if t < 1:
            raise ValueError(f"{len(times)} steps do not fit between t_start = {int(times[0])} and 1")
        out.append(t)
    return out


class InpaintSampler:
    def __init__(self, cfg, schedule: DiffusionSchedule, decoder):
        self.cfg, self.schedule, self.decoder = cfg, schedule, decoder
        self._dev_cache = {}

    def _coefs(self, times: List[int]):
        sab, s1m = self.schedule._host_t["sqrt_alpha_bar"], self.schedule._host_t["sqrt_one_minus_alpha_bar"]
        out = []
        for i, t in enumerate(times):
            t_next = times[i + 1] if i < len(times) - 1 else 0
            a = torch.tensor(float(self.schedule._host["alpha_bar"][t_next]), dtype=torch.float32)
            # sqrt(alpha_next), sqrt(1 - alpha_next) as fp32 tensor ops of the fp32 table value (inference_pipeline.py:131-132)
            out += [float(sab[t]), float(s1m[t]), float(torch.sqrt(a)), float(torch.sqrt(1 - a))]
        return out

    @staticmethod
    def _check_keep(keep, known_mel, overlap_len: int, noise_k, shape, n: int) -> None:
        """The argument rules of ``keep=`` for a call on ``shape`` = (B, T, n_mels) with ``n`` steps: ValueError, before any launch."""
        if keep is None:
            return
        B, T, M = (int(v) for v in shape)
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"keep must be a bool or uint8 tensor of shape [{B}, {T}], got "
                             f"{keep.dtype if isinstance(keep, torch.Tensor) else type(keep).__name__}")
        if tuple(keep.shape) != (B, T):
            raise ValueError(f"keep must be [{B}, {T}], got {list(keep.shape)}")
        if known_mel is None:
            raise ValueError("keep= needs known_mel (the mel whose kept frames are held)")
        if tuple(known_mel.shape) != (B, T, M):
            raise ValueError(f"with keep=, known_mel must be [{B}, {T}, {M}], got {list(known_mel.shape)}")
        if overlap_len != 0:
            raise ValueError(f"with keep=, overlap_len must be 0 (the mask says which frames are known), got {overlap_len}")
        if noise_k is not None and tuple(noise_k.shape) != (n, B, T, M):
            raise ValueError(f"with keep=, noise_k must be [{n}, {B}, {T}, {M}], got {list(noise_k.shape)}")

    @staticmethod
    def keep_mask(B: int, T: int, intervals, device=None) -> torch.Tensor:
        """The ``keep=`` mask of the in-painting samplers from frame intervals: ``intervals[b]`` is a sequence of half-open
        (start, end) pairs, 0 <= start <= end <= T, and frame f of row b is kept when it lies in one of them.  Returns a bool
        [B, T] tensor on ``device``.  ValueError for a list that is not B long or an interval outside [0, T]."""
        intervals = list(intervals)
        if len(intervals) != B:
            raise ValueError(f"intervals: expected {B} entries (one list of (start, end) pairs per row), got {len(intervals)}")
        mask = torch.zeros(B, T, dtype=torch.bool)
        for b, row in enumerate(intervals):
            for pair in row:
                try:
                    lo, hi = (int(v) for v in pair)
                except (TypeError, ValueError):
                    raise ValueError(f"intervals[{b}]: expected (start, end) pairs, got {pair!r}") from None
                if not 0 <= lo <= hi <= T:
                    raise ValueError(f"intervals[{b}]: need 0 <= start <= end <= {T}, got ({lo}, {hi})")
                mask[b, lo:hi] = True
        return mask if device is None else mask.to(device)

    def _run(self, x: torch.Tensor, sem_features: torch.Tensor, times: List[int], step_idx, known_mel, overlap_len: int,
             cfg_scale: float, noise_k, seed: int, x_lengths=None, sem_lengths=None, seeds=None, *, lms_rows=None,
             return_intermediates: bool = False, keep=None):
        """One C-ABI call (native.sample_inpaint): edtts_sample_inpaint_len, or with ``lms_rows`` (DPMSolverPP.step_coefficients of
        ``times``) edtts_sample_inpaint_multistep_len.  ``step_idx``: the constant step index, or "index" for 0 .. n-1.
        ``keep`` (bool or uint8 [B, T]): the known frames are those it names, of a ``known_mel`` [B, T, n_mels] -- the *_mask_len
        twin of either entry point."""
        dec = self.decoder
        B, T, M = x.shape
        S = sem_features.shape[1]
        self._check_keep(keep, known_mel, overlap_len, noise_k, (B, T, M), len(times))
        if (known_mel is not None and isinstance(x_lengths, torch.Tensor) and not x_lengths.is_cuda and B
                and int(x_lengths.min()) < overlap_len):
            raise ValueError(f"x_lengths: every utterance needs at least overlap_len = {overlap_len} frames, got {int(x_lengths.min())}")
        t_len = native.lengths(x_lengths, B, T, x.device, "x_lengths")
        s_len = native.lengths(sem_lengths, B, S, x.device, "sem_lengths")
        sd = None if seeds is None else native.seed_tensor(seeds, B, x.device)
        n = len(times)
        dev = x.device
        x = x.to(torch.float32).contiguous().clone()
        sem_features = sem_features.to(device=dev, dtype=torch.float32).contiguous()
        key = (tuple(times), step_idx, str(dev))
        cached = self._dev_cache.get(key)
        if cached is None:  # (device copies made once: no H2D copy at call time -> capturable; setdefault: one winner per key)
            # (both are synchronous host-to-device copies, so their contents are there for every stream)
            cached = self._dev_cache.setdefault(key, (torch.tensor(times, dtype=torch.int64, device=dev),
                                                      torch.tensor(list(range(n)) if step_idx == "index" else [step_idx] * n,
                                                                   dtype=torch.int64, device=dev)))
        t_all, s_all = cached
        packed = dec._ensure_packed()
        ws = dec.workspace(B, T, S, n, dev)
        guided = float(cfg_scale) != 1.0
        ws_u = dec.workspace(B, T, S, n, dev, tag="uncond") if guided else None
        zeros = torch.zeros_like(sem_features) if guided else None
        v_u = torch.empty_like(x) if guided else None
        if known_mel is not None:
            known_mel = known_mel.to(device=dev, dtype=torch.float32).contiguous()
            k_frames = T if keep is not None else overlap_len
            if tuple(known_mel.shape) != (B, k_frames, M):
                raise ValueError(f"known_mel must be [{B}, {k_frames}, {M}], got {tuple(known_mel.shape)}")
            if noise_k is not None:
                noise_k = noise_k.to(device=dev, dtype=torch.float32).contiguous()
                if tuple(noise_k.shape) != (n, B, k_frames, M):
                    raise ValueError(f"noise_k must be [{n}, {B}, {k_frames}, {M}]")
        else:
            noise_k = None
        if keep is not None:  # (a bool tensor is bytes of 0 / 1: reinterpreted, not converted; a device tensor is not copied)
            keep = keep.to(dev).contiguous()
            keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        x, x0_all = native.sample_inpaint(dec.dims(), packed, ws, ws_u, sem_features, zeros, x, t_all, s_all,
                                          self._coefs(times) if lms_rows is None else None, known_mel, overlap_len, noise_k, seed, cfg_scale,
                                          v_u, t_len, s_len, sd, lms_rows=lms_rows, want_intermediates=return_intermediates, keep=keep)
        return (x, list(x0_all.unbind(0))) if lms_rows is not None and return_intermediates else x

    @torch.no_grad()
    def inpaint_student_sample(self, x_shape, sem_features, known_mel=None, overlap_len: int = 0, num_steps: int = 4, *,
                               x_init: Optional[torch.Tensor] = None, noise_k: Optional[torch.Tensor] = None, seed: int = 0,
                               x_lengths: Optional[torch.Tensor] = None, sem_lengths: Optional[torch.Tensor] = None,
                               seeds: Optional[Sequence[int]] = None, keep: Optional[torch.Tensor] = None):
        """inference_pipeline.py:97-140.  ``x_init`` / ``noise_k`` inject the draws the reference takes from torch.randn /
        torch.randn_like (parity); otherwise the start noise comes from the library's Philox stream and the per-step q_sample
        noise from the in-kernel generator.

        Ragged batches: ``x_lengths`` / ``sem_lengths`` (int64 [B], see native.lengths) and ``seeds`` (B ints,
        or a device int64 [B] tensor) make row b bitwise the call on utterance b alone (its first x_lengths[b] frames and
        sem_lengths[b] feature rows, ``seed=seeds[b]``); frames past x_lengths[b] come out as exact zeros.

        ``keep`` (bool or uint8 [B, T]): the known frames are the ones it names, anywhere in the utterance,
        of a ``known_mel`` [B, T, n_mels]; ``overlap_len`` stays 0 and ``noise_k`` is [num_steps, B, T, n_mels].  Kept frames come
        out bitwise ``known_mel``; kept frames past x_lengths[b] are ignored; ``keep[b, f] = f < ov`` with ``seeds`` is bitwise the
        prefix call.  InpaintSampler.keep_mask builds the mask from frame intervals."""
        self._check_keep(keep, known_mel, overlap_len, noise_k, x_shape, num_steps)
        dev = sem_features.device
        if x_init is not None:
            x = x_init.to(dev)
        elif seeds is not None:  # row b = the solo call's start noise (a prefix of the row when the row is longer)
            x = native.randn_rows(tuple(x_shape), dev, seeds, stream_id=0x51)
        else:
            x = native.randn(tuple(x_shape), dev, seed=seed, stream_id=0x51)
        times = linspace_times(self.cfg.diff_steps - 1, num_steps)
        return self._run(x, sem_features, times, 3, known_mel, overlap_len if known_mel is not None else 0, 1.0, noise_k, seed,
                         x_lengths, sem_lengths, seeds, keep=keep)

    @torch.no_grad()
    def inpaint_teacher_refine(self, x_coarse, sem_features, known_mel=None, overlap_len: int = 0, strength: float = 0.2,
                               steps: int = 10, cfg_scale: float = 1.0, *, noise: Optional[torch.Tensor] = None,
                               noise_k: Optional[torch.Tensor] = None, seed: int = 0, x_lengths: Optional[torch.Tensor] = None,
                               sem_lengths: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None,
                               keep: Optional[torch.Tensor] = None):
        """inference_pipeline.py:145-196: q_sample(x_coarse, t_start = int(T * strength)) then ``steps`` guided v-prediction steps.
        ``x_lengths`` / ``sem_lengths`` / ``seeds`` / ``keep``: as inpaint_student_sample (with ``seeds`` the q_sample noise of row b
        is the solo call's)."""
        self._check_keep(keep, known_mel, overlap_len, noise_k, x_coarse.shape, steps)
        t_start = self._t_start(strength)
        x = self._refine_start(x_coarse, t_start, noise, seed, seeds)
        times = linspace_times(t_start, steps)
        return self._run(x, sem_features, times, 0, known_mel, overlap_len if known_mel is not None else 0, cfg_scale, noise_k, seed,
                         x_lengths, sem_lengths, seeds, keep=keep)

    def _t_start(self, strength: float) -> int:
        t_start = int(self.cfg.diff_steps * strength)
        if not 0 <= t_start < self.cfg.diff_steps:
            raise IndexError(f"t_start = int(diff_steps * strength) = {t_start} is outside the schedule tables "
                             "(the reference indexes them with it too)")
        return t_start

    def _refine_start(self, x_coarse, t_start: int, noise, seed: int, seeds) -> torch.Tensor:
        """q_sample(x_coarse, t_start) with injected, per-row or single-seed noise (inference_pipeline.py:160-163)."""
        dev = x_coarse.device
        if noise is not None:
            nz = noise.to(dev)
        elif seeds is not None:
            nz = native.randn_rows(tuple(x_coarse.shape), dev, seeds, stream_id=0x52)
        else:
            nz = native.randn(tuple(x_coarse.shape), dev, seed=seed, stream_id=0x52)
        key = ("q_sample", t_start, str(dev))
        cached = self._dev_cache.get(key)
        if cached is None:  # (device copies made once, as in _run: a call with device lengths and seeds is capturable)
            cached = self._dev_cache.setdefault(key, (self.schedule._host_t["sqrt_alpha_bar"][t_start].to(dev),
                                                      self.schedule._host_t["sqrt_one_minus_alpha_bar"][t_start].to(dev)))
        sab, s1m = cached
        return sab * x_coarse.to(torch.float32) + s1m * nz  # schedule.q_sample (schedule.py:81-84): plain torch on the device

    def dpm_plan(self, strength: float, steps: int, order: int):
        """(times, coefficient rows) of inpaint_dpm_refine, host only: DPMSolverPP(order, predict_x0=False).get_time_steps(steps,
        max_t=t_start), made strictly decreasing where they repeat (strictly_decreasing_times), and the solver's step_coefficients of
        those times.  ValueError for an order outside 1..3, steps < 1, or more steps than table rows below t_start."""
        if order not in (1, 2, 3):
            raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
        if int(steps) < 1:
            raise ValueError(f"steps must be >= 1, got {steps}")
        t_start = self._t_start(strength)
        if t_start < 1:
            raise ValueError(f"strength {strength}: t_start = {t_start}, DPM-Solver++ visits times in [1, t_start]")
        key = ("dpm_plan", t_start, int(steps), order)
        cached = self._dev_cache.get(key)
        if cached is None:
            solver = DPMSolverPP(self.schedule, order=order, predict_x0=False)
            solver.device = "cpu"  # (the times are host integers here; the device copy is _run's, made once)
            times = strictly_decreasing_times(solver.get_time_steps(int(steps), max_t=t_start).tolist())
            cached = self._dev_cache.setdefault(key, (times, solver.step_coefficients(times)))
        return cached

    @torch.no_grad()
    def inpaint_dpm_refine(self, x_coarse, sem_features, known_mel=None, overlap_len: int = 0, strength: float = 0.999,
                           steps: int = 15, order: int = 2, cfg_scale: float = 1.0, *, noise: Optional[torch.Tensor] = None,
                           noise_k: Optional[torch.Tensor] = None, seed: int = 0, x_lengths: Optional[torch.Tensor] = None,
                           sem_lengths: Optional[torch.Tensor] = None, seeds: Optional[Sequence[int]] = None, step_idx=0,
                           return_intermediates: bool = False, keep: Optional[torch.Tensor] = None):
        """inpaint_teacher_refine with DPM-Solver++'s multistep update (schedule.py: DPMSolverPP, v-prediction model) in place of the
        first-order step: the same start point q_sample(x_coarse, t_start), known-tail injection, guidance, lengths and seeds; the
        visiting times are DPMSolverPP.get_time_steps(steps, max_t=t_start) (strictly_decreasing_times of them), and each step's x0 = clamp(predict_x0_from_v) feeds the
        first / second / third_order_update over the x0 history (``order``).  One C-ABI call (edtts_sample_inpaint_multistep_len).
        ``step_idx``: the constant step index handed to the decoder (0: the long-form pipeline's), or "index" for 0 .. steps-1
        (DPMSolverPP.sample's convention).  ``return_intermediates``: also return the list of every step's x0.
        ``keep``: as inpaint_student_sample (edtts_sample_inpaint_multistep_mask_len: each step's q_sample of the kept frames is a
        small launch of its own between the steps)."""
        times, rows = self.dpm_plan(strength, steps, order)
        self._check_keep(keep, known_mel, overlap_len, noise_k, x_coarse.shape, len(times))
        if step_idx != "index" and not isinstance(step_idx, int):
            raise ValueError(f"step_idx must be an int or \"index\", got {step_idx!r}")
        if known_mel is not None and overlap_len > x_coarse.shape[1]:
            raise ValueError(f"overlap_len = {overlap_len} exceeds the {x_coarse.shape[1]} frames of x_coarse")
        x = self._refine_start(x_coarse, self._t_start(strength), noise, seed, seeds)
        return self._run(x, sem_features, times, step_idx, known_mel, overlap_len if known_mel is not None else 0, cfg_scale, noise_k,
                         seed, x_lengths, sem_lengths, seeds, lms_rows=rows, return_intermediates=return_intermediates, keep=keep)

    @torch.no_grad()
    def edit(self, mel_n: torch.Tensor, sem_features: torch.Tensor, regenerate, *, num_steps: int = 4, refine: Optional[str] = "dpmpp",
             steps: Optional[int] = None, order: int = 2, strength: Optional[float] = None, cfg_scale: float = 1.0,
             x_lengths: Optional[torch.Tensor] = None, sem_lengths: Optional[torch.Tensor] = None,
             seeds: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Re-synthesise stretches of an utterance and keep the rest (speech editing: ``sem_features`` are the edited utterance's
        features, ``mel_n`` [B, T, n_mels] its normalised mel before the edit).  ``regenerate[b]``: half-open (start, end) frame
        intervals of row b to synthesise anew (keep_mask's format); every other frame is kept, bitwise, with context on both sides.
        The student sample (``num_steps``) under that mask, then the refinement under the same mask: ``refine="dpmpp"``
        (inpaint_dpm_refine; ``steps`` 15, ``order``, ``strength`` 0.999 unless given), ``"ddim"`` (inpaint_teacher_refine; ``steps``
        10, ``strength`` 0.2 unless given) or None (the student sample is returned).  ``cfg_scale`` guides the refinement.
        ValueError for another ``refine``, before any launch."""
        if refine not in SOLVERS + (None,):
            raise ValueError(f"refine must be one of {SOLVERS} or None, got {refine!r}")
        B, T, M = mel_n.shape
        keep = ~self.keep_mask(B, T, regenerate, mel_n.device)
        if refine == "dpmpp":  # (the refinement's own argument errors, before the student sample runs)
            strength, steps = 0.999 if strength is None else strength, 15 if steps is None else steps
            self.dpm_plan(strength, steps, order)
        elif refine == "ddim":
            strength, steps = 0.2 if strength is None else strength, 10 if steps is None else steps
            self._t_start(strength)
        kw = dict(x_lengths=x_lengths, sem_lengths=sem_lengths, seeds=seeds, keep=keep)
        x = self.inpaint_student_sample((B, T, M), sem_features, mel_n, 0, num_steps, **kw)
        if refine == "dpmpp":
            return self.inpaint_dpm_refine(x, sem_features, mel_n, 0, strength, steps, order, cfg_scale, **kw)
        if refine == "ddim":
            return self.inpaint_teacher_refine(x, sem_features, mel_n, 0, strength, steps, cfg_scale, **kw)
        return x

    @staticmethod
    def latent_slices(n_chunks: int, hop_samples: int, chunk_samples: int, sample_rate: int) -> List[tuple]:
        """Per-chunk [start_lat, end_lat) into the global semantic features (inference_pipeline.py:308-317): sample position ->
        seconds -> 16 kHz sample -> HuBERT frame (320 samples each), with the reference's float arithmetic and truncations."""
        out = []
        for i in range(n_chunks):
            start_sample = i * hop_samples
            end_sample = start_sample + chunk_samples
            out.append((int(start_sample / sample_rate * 16000) // 320, int(end_sample / sample_rate * 16000) // 320))
        return out

    @staticmethod
    def chunk_plan(total_frames: int, chunk_frames: int, overlap_frames: int, hop_length: int, chunk_samples: Optional[int] = None,
                   overlap_samples: Optional[int] = None, total_samples: Optional[int] = None):
        """(n_chunks, chunk_samples, hop_samples) of the sliding window, inference_pipeline.py:221-225: the sample counts are used
        verbatim when given (the reference fixes THEM and derives the frame counts), else rebuilt as frames * hop_length."""
        chunk_samples = int(chunk_samples) if chunk_samples is not None else chunk_frames * hop_length
        overlap_samples = int(overlap_samples) if overlap_samples is not None else overlap_frames * hop_length
        total_samples = int(total_samples) if total_samples is not None else total_frames * hop_length
        hop_samples = chunk_samples - overlap_samples
        if hop_samples <= 0:
            raise ValueError(f"need overlap_samples < chunk_samples, got {overlap_samples} / {chunk_samples}")
        n_chunks = max(1, -(-(total_samples - overlap_samples) // hop_samples))  # int(np.ceil(...)), :225
        return n_chunks, chunk_samples, hop_samples

    @staticmethod
    def chunk_stats_from_audio(wavs, chunk_samples: int, overlap_samples: int, mel):
        """Per utterance the per-chunk (mean, std) pairs that generate_long_batch(..., chunk_stats=...) takes, from the utterances'
        audio (inference_pipeline.py:354-355) -- audio.chunk_stats_from_audio: one launch for all chunks of all utterances."""
        from .audio import chunk_stats_from_audio
        return chunk_stats_from_audio(wavs, chunk_samples, overlap_samples, mel)

    @torch.no_grad()
    def generate_long(self, sem_features: torch.Tensor, total_frames: int, chunk_frames: int, overlap_frames: int,
                      chunk_stats, *, strength: float = 0.999, steps: int = 10, cfg_scale: float = 1.0, seed: int = 0,
                      latent_slices: Optional[List[tuple]] = None, hop_length: Optional[int] = None,
                      sample_rate: Optional[int] = None, draws: Optional[List[dict]] = None,
                      chunk_samples: Optional[int] = None, overlap_samples: Optional[int] = None,
                      total_samples: Optional[int] = None, solver: str = "ddim", order: int = 2) -> torch.Tensor:
        """The reference's context-aware sliding window (inference_pipeline.py:296-367), statement for statement:

            for chunk i (hop = chunk_frames - overlap_frames frames apart):
                z_q_chunk   = sem_features[:, start_lat:end_lat]                                         (:308-325)
                x_refined   = inpaint_teacher_refine(randn, z_q_chunk, known_mel=prev_mel_tail, overlap_len=overlap_frames, ...)
                prev_tail   = x_refined[:, -overlap_frames:]                                             (:346)
                mel_denorm  = denormalize_mel(x_refined, mean_i, std_i)         per-chunk statistics     (:349-352)
                lin_mel     = exp(mel_denorm)^T                                  LINEAR mel [n_mels, T]   (:353)
                final[:, f0:f0+chunk] += lin_mel * window ;  weights[:, f0:f0+chunk] += window           (:360-361)
            final = (final / clamp(weights, 1e-5))[:, :total_frames]                                     (:364-367)

        with the trapezoid window of :253-260 (linear fade-in over the first and fade-out over the last ``overlap_frames``
        frames).  Returns the stitched LINEAR mel [n_mels, total_frames] -- what the reference hands to its smoothing /
        InverseMelScale / Griffin-Lim tail (:376-399), which is ``MelVocoder.from_linear([mel])`` (melpost.py; it takes the whole
        list that ``generate_long_batch`` returns in one call).

        ``chunk_stats``: one (mean, std) pair per chunk, each broadcastable to [1, 1, n_mels] -- the reference takes them from the
        ground-truth audio of the chunk (normalize_mel of its log-mel, :349-351); that audio front end (torchaudio) is outside the
        path, so the caller supplies the numbers.  ``latent_slices``: the per-chunk [start, end) rows of ``sem_features``; by
        default computed from ``hop_length`` / ``sample_rate`` (cfg values) exactly as the reference does.  ``draws`` (parity
        tests): per chunk a dict with the reference's torch.randn draws ``x_coarse``, ``noise`` and (chunks with a known tail)
        ``noise_k``; otherwise they come from the library's Philox streams.
        ``chunk_samples`` / ``overlap_samples`` / ``total_samples``: the reference works the other way round -- it FIXES the sample
        counts (int(2.0 s * sample_rate), int(0.5 s * sample_rate), wav.shape[1]; :221-225) and derives the frame counts through a
        centred mel transform (frames = samples // hop + 1: 201 / 51 frames for 32000 / 8000 samples at hop 160), so frames * hop
        over-states them (8160 instead of 8000 overlap samples) and the chunk count can come out one short.  A caller that mirrors
        the reference passes its sample counts here and they are used verbatim for the chunk count and the semantic slices; the
        defaults (frames * hop_length) serve callers that think in frames.
        The chunk loop is sequential by construction (chunk i is conditioned on the tail of chunk i-1).
        This is generate_long_batch of one utterance (same results): every check runs before the first chunk, the messages name
        "utterance 0", and a ``latent_slices`` or ``draws`` list shorter than the chunk count is a ValueError (an IndexError at
        that chunk before).
        ``solver`` / ``order``: "ddim" is the reference's first-order step (inpaint_teacher_refine); "dpmpp" refines every chunk with
        inpaint_dpm_refine at that order -- fewer steps for the same trajectory length, everything around the per-chunk call as is."""
        return self.generate_long_batch([sem_features], [total_frames], chunk_frames, overlap_frames, [chunk_stats], seeds=[seed],
                                        strength=strength, steps=steps, cfg_scale=cfg_scale,
                                        latent_slices=None if latent_slices is None else [latent_slices], hop_length=hop_length,
                                        sample_rate=sample_rate, draws=None if draws is None else [draws], chunk_samples=chunk_samples,
                                        overlap_samples=overlap_samples,
                                        total_samples=None if total_samples is None else [total_samples], solver=solver, order=order)[0]

    def plan_long_batch(self, sem_rows: Sequence[int], total_frames: Sequence[int], chunk_frames: int, overlap_frames: int,
                        chunk_stats: Sequence, seeds: Sequence[int], *, latent_slices=None, hop_length: Optional[int] = None,
                        sample_rate: Optional[int] = None, draws=None, chunk_samples: Optional[int] = None,
                        overlap_samples: Optional[int] = None, total_samples=None) -> List[dict]:
        """The checks and the chunk plan of generate_long_batch, host only: per utterance a dict with ``n_chunks`` and ``slices`` (the
        [start, end) feature rows of each chunk, clipped to the utterance's ``sem_rows``).  Raises what generate_long raises, naming the
        utterance."""
        N = len(sem_rows)

        def per_utt(name, v, required):
            if v is None:
                if required:
                    raise ValueError(f"{name}: one entry per utterance is required")
                return [None] * N
            v = list(v)
            if len(v) != N:
                raise ValueError(f"{name}: expected {N} entries (one per utterance), got {len(v)}")
            return v
        total_frames = per_utt("total_frames", total_frames, True)
        chunk_stats = per_utt("chunk_stats", chunk_stats, True)
        seeds = per_utt("seeds", seeds, True)
        latent_slices = per_utt("latent_slices", latent_slices, False)
        draws = per_utt("draws", draws, False)
        total_samples = per_utt("total_samples", total_samples, False)
        if not 0 <= overlap_frames < chunk_frames:
            raise ValueError(f"need 0 <= overlap_frames < chunk_frames, got {overlap_frames} / {chunk_frames}")
        hop_frames = chunk_frames - overlap_frames
        hop_length = int(hop_length if hop_length is not None else self.cfg.hop_length)
        sample_rate = int(sample_rate if sample_rate is not None else self.cfg.sample_rate)
        plans = []
        for n in range(N):
            try:
                n_chunks, c_samples, hop_samples = self.chunk_plan(total_frames[n], chunk_frames, overlap_frames, hop_length, chunk_samples,
                                                                    overlap_samples, total_samples[n])
            except ValueError as e:
                raise ValueError(f"utterance {n}: {e}") from None
            if len(chunk_stats[n]) != n_chunks:
                raise ValueError(f"utterance {n}: chunk_stats must hold {n_chunks} (mean, std) pairs, got {len(chunk_stats[n])}")
            sl = latent_slices[n] if latent_slices[n] is not None else self.latent_slices(n_chunks, hop_samples, c_samples, sample_rate)
            if len(sl) < n_chunks:
                raise ValueError(f"utterance {n}: latent_slices must hold {n_chunks} (start, end) pairs, got {len(sl)}")
            if draws[n] is not None and len(draws[n]) < n_chunks:
                raise ValueError(f"utterance {n}: draws must hold {n_chunks} dicts, got {len(draws[n])}")
            if (n_chunks - 1) * hop_frames + chunk_frames > total_frames[n] + 1000:  # :227 (room for the last, ragged chunk)
                raise ValueError(f"utterance {n}: chunk geometry exceeds the reference's stitching buffer (total_frames + 1000 frames)")
            rows = int(sem_rows[n])
            slices = []
            for i in range(n_chunks):
                l0, l1 = (int(v) for v in sl[i])
                a, b = range(rows)[l0:l1].start, range(rows)[l0:l1].stop  # what sem_features[:, l0:l1] selects
                if b <= a:
                    raise ValueError(f"utterance {n}: chunk {i}: empty semantic slice [{l0}:{l1}] of {rows} rows")
                slices.append((a, b))
            plans.append({"n_chunks": n_chunks, "slices": slices})
        return plans

    @torch.no_grad()
    def generate_long_batch(self, sem_features: Sequence[torch.Tensor], total_frames: Sequence[int], chunk_frames: int,
                            overlap_frames: int, chunk_stats: Sequence, *, seeds: Sequence[int], strength: float = 0.999,
                            steps: int = 10, cfg_scale: float = 1.0, latent_slices: Optional[Sequence] = None,
                            hop_length: Optional[int] = None, sample_rate: Optional[int] = None, draws: Optional[Sequence] = None,
                            chunk_samples: Optional[int] = None, overlap_samples: Optional[int] = None,
                            total_samples: Optional[Sequence[int]] = None, solver: str = "ddim", order: int = 2) -> List[torch.Tensor]:
        """generate_long for N utterances at once.  Lists with one entry per utterance: ``sem_features`` ([1, S_n, semantic_dim]),
        ``total_frames``, ``chunk_stats`` (that utterance's per-chunk (mean, std) pairs), ``seeds`` and, optionally,
        ``total_samples``, ``latent_slices`` and ``draws``; the other arguments are generate_long's and shared.  Returns one
        [n_mels, total_frames_n] LINEAR mel per utterance, in the caller's order.

        Contract: entry n is bitwise generate_long(sem_features[n], total_frames[n], ..., seed=seeds[n]) with that utterance's own
        total_samples / latent_slices / draws.

        The chunk loop runs in lockstep over the chunk index i.  The utterances are sorted by chunk count, so those that still have
        a chunk i are a prefix of the batch; their chunk i is ONE inpaint_teacher_refine call of B = that many rows, S = the longest
        of their semantic slices and sem_lengths = each row's own slice length, with per-row seeds seeds[n] + 2 i (q_sample noise)
        and seeds[n] + 2 i + 1 (coarse start noise), each row conditioned on its own previous tail.  Rows whose ``draws`` supply
        different keys at chunk i (parity runs) go in separate calls.  ``solver="dpmpp"`` makes that call inpaint_dpm_refine at
        ``order`` (same planning, seeds and stitching).  The stitch is batched tensor arithmetic on an
        [N, n_mels, max(total_frames) + 1000] buffer; all live rows of chunk i start at frame i * (chunk_frames - overlap_frames)."""
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        dpm_order = order  # (`order` below is the utterances' order)
        if solver == "dpmpp":
            self.dpm_plan(strength, steps, dpm_order)  # (its ValueErrors, before the first chunk)
        N = len(sem_features)
        if N == 0:
            return []
        for n, f in enumerate(sem_features):
            if f.dim() != 3 or f.shape[0] != 1:
                raise ValueError(f"utterance {n}: sem_features must be [1, S, semantic_dim], got {list(f.shape)}")
        plans = self.plan_long_batch([f.shape[1] for f in sem_features], total_frames, chunk_frames, overlap_frames, chunk_stats, seeds,
                                     latent_slices=latent_slices, hop_length=hop_length, sample_rate=sample_rate, draws=draws,
                                     chunk_samples=chunk_samples, overlap_samples=overlap_samples, total_samples=total_samples)
        dev = sem_features[0].device
        M = self.cfg.n_mels
        hop_frames = chunk_frames - overlap_frames
        order = sorted(range(N), key=lambda n: -plans[n]["n_chunks"])  # (stable) the live utterances of every chunk are a prefix
        width = max(int(v) for v in total_frames) + 1000
        final = torch.zeros(N, M, width, device=dev)
        weights = torch.zeros(N, 1, width, device=dev)
        window = torch.ones(1, chunk_frames, device=dev)
        if overlap_frames > 0:  # (:253-260; with no overlap the window is flat and no tail is handed on)
            window[0, :overlap_frames] = torch.linspace(0, 1, overlap_frames, device=dev)
            window[0, -overlap_frames:] = torch.linspace(1, 0, overlap_frames, device=dev)
        prev_tail = None
        for i in range(plans[order[0]]["n_chunks"]):
            live = [n for n in order if plans[n]["n_chunks"] > i]
            k = len(live)
            rows = [plans[n]["slices"][i] for n in live]
            lens = [b - a for a, b in rows]
            S = max(lens)
            if k == 1:
                sem = sem_features[live[0]][:, rows[0][0]:rows[0][1]].to(torch.float32).contiguous()
            else:
                sem = torch.zeros(k, S, sem_features[live[0]].shape[2], dtype=torch.float32, device=dev)
                for j, (n, (a, b)) in enumerate(zip(live, rows)):
                    sem[j, :b - a] = sem_features[n][0, a:b]
            # (device tensors, queued without a host stall; the values are in [1, S] by construction)
            s_len = None if min(lens) == S else native.host_to_device(torch.tensor(lens, dtype=torch.int64), dev)
            # rows that inject different reference draws at this chunk run in separate calls (one call when nobody injects)
            d = [draws[n][i] if draws is not None and draws[n] is not None else {} for n in live]
            groups = {}
            for j in range(k):
                groups.setdefault(tuple(sorted(d[j])), []).append(j)
            x = torch.empty(k, chunk_frames, M, device=dev) if len(groups) > 1 else None
            for keys, J in groups.items():
                whole = len(J) == k
                pick = (lambda t: t) if whole else (lambda t: t[J])
                sd = native.seed_tensor([seeds[live[j]] + 2 * i for j in J], len(J), dev)
                if "x_coarse" in keys:
                    x_coarse = torch.cat([d[j]["x_coarse"].to(dev) for j in J])
                else:
                    x_coarse = native.randn_rows((len(J), chunk_frames, M), dev,
                                                 native.seed_tensor([seeds[live[j]] + 2 * i + 1 for j in J], len(J), dev), stream_id=0x53)
                noise = torch.cat([d[j]["noise"].to(dev) for j in J]) if "noise" in keys else None
                noise_k = torch.cat([d[j]["noise_k"].to(dev) for j in J], dim=1) if "noise_k" in keys and prev_tail is not None else None
                known = None if prev_tail is None else pick(prev_tail[:k])
                sl = None if s_len is None else pick(s_len)
                ov = overlap_frames if known is not None else 0
                if solver == "dpmpp":
                    xg = self.inpaint_dpm_refine(x_coarse, pick(sem).contiguous(), known, ov, strength, steps, dpm_order, cfg_scale,
                                                 noise=noise, noise_k=noise_k, sem_lengths=sl, seeds=sd)
                else:
                    xg = self.inpaint_teacher_refine(x_coarse, pick(sem).contiguous(), known, ov, strength, steps, cfg_scale,
                                                     noise=noise, noise_k=noise_k, sem_lengths=sl, seeds=sd)
                if whole:
                    x = xg
                else:
                    x[J] = xg
            prev_tail = x[:, -overlap_frames:].clone() if overlap_frames > 0 else None
            mean = torch.cat([torch.broadcast_to(torch.as_tensor(chunk_stats[n][i][0], dtype=torch.float32, device=dev), (1, 1, M))
                              for n in live])
            std = torch.cat([torch.broadcast_to(torch.as_tensor(chunk_stats[n][i][1], dtype=torch.float32, device=dev), (1, 1, M))
                             for n in live])
            lin = torch.exp(x * std + mean).transpose(1, 2)  # utils/audio.py:17-19, then :353-354
            f0 = i * hop_frames
            final[:k, :, f0:f0 + chunk_frames] += lin * window
            weights[:k, :, f0:f0 + chunk_frames] += window
        out = final / torch.clamp(weights, min=1e-5)
        res = [None] * N
        for j, n in enumerate(order):
            res[n] = out[j, :, :int(total_frames[n])]
        return res
