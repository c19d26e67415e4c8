"""DiffusionObjective -- what stands between the decoder's prediction and the optimiser, on the library's kernels.

Every trainer of the reference runs, around the decoder call: ``normalize_mel``, ``torch.randn_like``, ``schedule.q_sample``,
``schedule.get_v_target``, ``F.mse_loss`` and the logging metrics ``predict_x0_from_v`` / ``F.mse_loss`` / ``F.cosine_similarity``,
each ended by ``.item()`` (train_v2.py:107-163; edge_diffusion_tts/train.py:143-158), and in the later stages
``ConsistencyTrainer.progressive_distillation_loss`` and ``consistency_loss`` (training/consistency.py:60-122).  Here that is
``prepare`` (two launches) and one of the losses (two launches, one more in the backward), with per-utterance lengths and with noise
from the library's Philox streams.  Nothing synchronises and there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from . import native
from ._cache import WorkspaceCache

__all__ = ["DiffusionObjective", "PreparedBatch"]

_KINDS = {"v": native.EDTTS_OBJ_V, "eps": native.EDTTS_OBJ_EPS}


class PreparedBatch:
    """What ``DiffusionObjective.prepare`` returns: ``x_t`` [B, T, M] (what the decoder takes, 0 past the lengths), ``mean`` / ``std``
    [B, 1, M] (None with ``normalize=False``), ``t``, ``seeds`` (device int64 [B], None with injected noise) and ``lengths`` (device
    int64 [B] or None).  With ``parts=True`` also ``mel_n``, ``noise`` and ``target``.  The losses rebuild mel_n, the noise and x_t
    from the batch (the raw mel, the statistics, the seeds) instead of reading them back, so the raw mel must stay as it is until the
    loss has run."""
    __slots__ = ("x_t", "mean", "std", "t", "seeds", "lengths", "mel_n", "noise", "target", "batch")

    def __init__(self, batch: native.ObjBatch, x_t, mel_n=None, noise=None, target=None):
        self.batch = batch
        self.x_t, self.mean, self.std, self.t, self.seeds, self.lengths = x_t, batch.mean, batch.std, batch.t, batch.seeds, batch.lengths
        self.mel_n, self.noise, self.target = mel_n, noise, target


class _ObjectiveLoss(torch.autograd.Function):
    """One edtts_objective_loss call.  Differentiable in ``pred`` and, for the consistency loss, in ``pred2`` (its reconstruction
    term only); a teacher's prediction gets no gradient.  The backward is ``unit * grad_output`` on the device."""

    @staticmethod
    def forward(ctx, pred, pred2, obj, kind, prep, t2, want1, want2):
        p1 = pred.detach().contiguous()
        p2 = None if pred2 is None else pred2.detach().contiguous()
        t_max = max(p1.shape[1], p1.shape[1] if p2 is None else p2.shape[1])
        out, unit, unit2 = native.objective_loss(kind, prep.batch, p1, p2, t2, want1, want2, obj.scratch(prep.batch.B, t_max, prep.batch.M, p1.device))
        ctx.units = (unit, unit2)
        obj.last_metrics = {"x0_mse": out[4], "x0_cos": out[5], "terms": out[1:4]}
        return out[0]

    @staticmethod
    def backward(ctx, grad):
        unit, unit2 = ctx.units
        g = grad.to(torch.float32).contiguous()
        return (None if unit is None else native.objective_scale(unit, g), None if unit2 is None else native.objective_scale(unit2, g),
                None, None, None, None, None, None)


class DiffusionObjective:
    """``prepare`` -> the decoder -> ``loss`` / ``distill_loss`` / ``consistency_loss`` -> ``backward()``.

    ``prediction``: what the decoder predicts, "v" (train_v2.py, the consistency stage) or "eps" (train.py phase 1).
    ``normalize``: True -- ``prepare`` takes the raw log-mel and applies ``normalize_mel`` (mean and unbiased std over the frames,
    clamped at 1e-5; over each row's own frames with ``lengths``); False -- the mel is already normalised.
    ``generator``: the CPU ``torch.Generator`` that ``prepare`` draws a 63-bit seed per row from when neither ``seeds`` nor ``noise``
    is given (None: torch's default CPU generator, so ``torch.manual_seed`` makes a run repeatable), as the decoder's
    ``dropout_generator``.
    ``last_metrics``: after each loss ``{"x0_mse", "x0_cos"}`` of train_v2.py:149-154 as 0-dim device tensors and ``"terms"``, the
    loss's three terms as means (unused ones 0) -- nothing is read back to the host.
    Every tensor is a contiguous fp32 (``t``, ``lengths``, seeds: int64) tensor on one HIP device; anything else raises."""

    WORKSPACE_CACHE = 8

    def __init__(self, schedule, prediction: str = "v", normalize: bool = True):
        if prediction not in _KINDS:
            raise ValueError(f"prediction: expected 'v' or 'eps', got {prediction!r}")
        self.schedule = schedule
        self.prediction = prediction
        self.kind = _KINDS[prediction]
        self.normalize = bool(normalize)
        self.generator: Optional[torch.Generator] = None
        self.last_metrics: dict = {}
        self._tables: dict = {}
        self._ws = WorkspaceCache()

    # ------------------------------------------------------------------------------------------ host state
    def _schedule_tables(self, device) -> torch.Tensor:
        """fp32 [4, T_diff] on ``device``: the four tables the kernels index by t (built once per device, not while capturing)."""
        key = str(device)
        tab = self._tables.get(key)
        if tab is None:
            s = self.schedule
            tab = torch.stack([getattr(s, n).detach().to("cpu", torch.float32) for n in (
                "sqrt_alpha_bar", "sqrt_one_minus_alpha_bar", "sqrt_recip_alpha_bar", "sqrt_recip_alpha_bar_minus_one")]).contiguous()
            tab = self._tables[key] = native.host_to_device(tab, device)
        return tab

    def scratch(self, B: int, T: int, M: int, device) -> torch.Tensor:
        """The loss kernels' partial sums for one (B, T, M, device, stream): WorkspaceCache's rules, as the decoder's workspace."""
        dev = torch.device(device)
        return self._ws.get(self, (B, T, M, str(dev)), dev, None,
                            lambda: torch.empty(native.objective_scratch_bytes(B, T, M), dtype=torch.uint8, device=dev))

    def release_pinned_workspaces(self) -> int:
        """Drop the workspaces pinned by captured graphs, once those graphs are gone (WorkspaceCache.release_pinned)."""
        return self._ws.release_pinned(lambda k: True)

    @staticmethod
    def _check(x, what: str, dtype=torch.float32, shape=None) -> None:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"DiffusionObjective: {what}: expected a tensor, got {type(x).__name__}")
        if x.dtype != dtype:
            raise ValueError(f"DiffusionObjective: {what}: expected dtype {dtype}, got {x.dtype}")
        if shape is not None and tuple(x.shape) != tuple(shape):
            raise ValueError(f"DiffusionObjective: {what}: expected shape {list(shape)}, got {list(x.shape)}")

    @staticmethod
    def _on_device(x, what: str, dev=None) -> None:
        if not x.is_cuda:
            raise native.EdttsError(f"DiffusionObjective: {what}: expected a tensor on the HIP device, got {x.device} -- there is no CPU fallback")
        if dev is not None and x.device != dev:
            raise native.EdttsError(f"DiffusionObjective: {what}: on {x.device}, the call runs on {dev}")

    # ------------------------------------------------------------------------------------------ prepare
    def prepare(self, mel: torch.Tensor, t: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                seeds: Union[None, Sequence[int], torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                stats: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, *, like: Optional[PreparedBatch] = None,
                parts: bool = False) -> PreparedBatch:
        """x_t = sqrt_alpha_bar[t] mel_n + sqrt_one_minus_alpha_bar[t] noise for mel [B, T, M] and t int64 [B].

        ``lengths`` (int64 [B], see ``native.lengths``): per-utterance frame counts; statistics, noise and every later mean run over
        each row's own frames and ``x_t`` is 0 past them.  ``stats=(mean, std)`` ([B, 1, M] each) replaces the computed statistics.
        Noise: ``noise=`` injects a tensor [B, T, M]; otherwise row b's noise is the first T M draws of the Philox stream
        (seeds[b], 0x54), bitwise ``native.randn_rows((B, T * M), seeds, stream_id=0x54)``; with neither, the seeds are drawn from
        ``self.generator`` on the host.  ``like=``: another prepared batch of the same mel whose statistics, seeds (or noise) and
        lengths are reused -- the consistency loss's "same noise, two timesteps".  ``parts``: also return mel_n, noise and target."""
        self._check(mel, "mel")
        if mel.dim() != 3:
            raise ValueError(f"DiffusionObjective: mel: expected [B, T, n_mels], got {list(mel.shape)}")
        B, T, M = mel.shape
        self._check(t, "t", torch.int64, (B,))
        if like is not None:
            if lengths is not None or seeds is not None or noise is not None or stats is not None:
                raise ValueError("DiffusionObjective: like= brings the lengths, the noise and the statistics; give none of them")
            if (like.batch.B, like.batch.T, like.batch.M) != (B, T, M):
                raise ValueError(f"DiffusionObjective: like= was prepared for {[like.batch.B, like.batch.T, like.batch.M]}, mel is {[B, T, M]}")
            lengths, seeds, noise = like.lengths, like.seeds, like.batch.noise
            stats = None if like.mean is None else (like.mean, like.std)
        if noise is not None:
            self._check(noise, "noise", torch.float32, (B, T, M))
        if stats is not None:
            if not self.normalize:
                raise ValueError("DiffusionObjective: normalize=False takes no statistics")
            for name, s in zip(("mean", "std"), stats):
                self._check(s, name, torch.float32, (B, 1, M))
        if seeds is not None and not isinstance(seeds, torch.Tensor) and len(seeds) != B:
            raise ValueError(f"DiffusionObjective: seeds: expected {B} seeds (one per row), got {len(seeds)}")
        dev = mel.device
        self._on_device(mel, "mel")
        self._on_device(t, "t", dev)
        if not mel.is_contiguous():
            raise native.EdttsError("DiffusionObjective: mel: tensor must be contiguous")
        lengths = native.lengths(lengths, B, T, dev, "lengths")
        if noise is not None:
            self._on_device(noise, "noise", dev)
            seeds = None
        else:
            if seeds is None:  # (a host draw from a CPU generator: no device work, no synchronisation)
                seeds = torch.randint(0, 2 ** 63 - 1, (B,), dtype=torch.int64, generator=self.generator)
            seeds = native.seed_tensor(seeds, B, dev)
        mean = std = None
        if self.normalize:
            mean, std = stats if stats is not None else native.objective_stats(mel, lengths)
        batch = native.ObjBatch(mel, t.contiguous(), self._schedule_tables(dev), mean, std, lengths, seeds, noise)
        out = native.objective_prepare(batch, self.kind, parts)
        return PreparedBatch(batch, *out) if parts else PreparedBatch(batch, out)

    # ------------------------------------------------------------------------------------------ the losses
    def _pred(self, pred, what: str, prep: PreparedBatch) -> None:
        self._check(pred, what)
        if pred.dim() != 3 or pred.shape[0] != prep.batch.B or pred.shape[2] != prep.batch.M:
            raise ValueError(f"DiffusionObjective: {what}: expected [{prep.batch.B}, T_pred, {prep.batch.M}], got {list(pred.shape)}")
        self._on_device(pred, what, prep.batch.mel.device)

    def loss(self, pred: torch.Tensor, prep: PreparedBatch) -> torch.Tensor:
        """``F.mse_loss(pred, target)`` of train_v2.train_step ("v": get_v_target) / train.py phase 1 ("eps": the noise) over the
        first min(T_pred, T) frames -- with lengths, over the live elements.  A 0-dim fp32 device tensor."""
        self._pred(pred, "pred", prep)
        return _ObjectiveLoss.apply(pred, None, self, self.kind, prep, None, torch.is_grad_enabled() and pred.requires_grad, False)

    def distill_loss(self, pred: torch.Tensor, teacher_pred: torch.Tensor, prep: PreparedBatch) -> torch.Tensor:
        """``progressive_distillation_loss`` with a teacher: mse of the two ``predict_x0_from_v`` values; no gradient to the teacher."""
        self._v_only("distill_loss")
        self._pred(pred, "pred", prep)
        self._pred(teacher_pred, "teacher_pred", prep)
        return _ObjectiveLoss.apply(pred, teacher_pred.detach(), self, native.EDTTS_OBJ_DISTILL, prep, None,
                                    torch.is_grad_enabled() and pred.requires_grad, False)

    def consistency_loss(self, pred1: torch.Tensor, prep1: PreparedBatch, pred2: torch.Tensor, prep2: PreparedBatch) -> torch.Tensor:
        """``ConsistencyTrainer.consistency_loss``: mse(x0_1, x0_2.detach()) + 0.5 (mse(x0_1, mel_n) + mse(x0_2, mel_n)); ``prep2``
        comes from ``prepare(mel, t2, like=prep1)``.  ``pred1`` receives the gradient of all three terms, ``pred2`` only that of
        its reconstruction term.  The metrics are those of ``pred1``."""
        self._v_only("consistency_loss")
        self._pred(pred1, "pred1", prep1)
        self._pred(pred2, "pred2", prep1)
        a, b = prep1.batch, prep2.batch
        same = lambda x, y: (x is None and y is None) or (x is not None and y is not None and x.data_ptr() == y.data_ptr())
        if not (same(a.mel, b.mel) and same(a.mean, b.mean) and same(a.seeds, b.seeds) and same(a.noise, b.noise) and same(a.lengths, b.lengths)):
            raise ValueError("DiffusionObjective: consistency_loss: prep2 must come from prepare(mel, t2, like=prep1)")
        on = torch.is_grad_enabled()
        return _ObjectiveLoss.apply(pred1, pred2, self, native.EDTTS_OBJ_CONSISTENCY, prep1, prep2.t, on and pred1.requires_grad,
                                    on and pred2.requires_grad)

    def _v_only(self, what: str) -> None:
        if self.prediction != "v":
            raise ValueError(f"DiffusionObjective: {what} is defined for prediction='v' (predict_x0_from_v), not {self.prediction!r}")
