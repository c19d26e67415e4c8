"""Semantic encoder -- API mirror of the reference's models/encoder.py, models/fsq.py and models/vq.py on MI355X.

The trained head after HuBERT (``proj``: Linear, GELU, LayerNorm, [Dropout], Linear; then the FSQ or VQ quantizer) runs as ONE
kernel per call (edtts_sem_encode, csrc/edtts_semantic.h): features in, token ids, z_q and per-code usage counts out.  Module
names and state-dict keys are the reference's, so its checkpoints and its own loading lines work unchanged.

HuBERT is a frozen third-party model and stays PyTorch plumbing: pass any module called as ``hubert(wav, output_hidden_states=True)``
that returns ``.hidden_states`` (transformers' ``HubertModel`` is one).  Without one, the first waveform call loads
``HubertModel.from_pretrained(cfg.hubert_id, local_files_only=True)`` from the local cache -- never from the network -- and raises
if it is not there.  Precomputed features ([B, T_feat, 768], as data/dataset_precomputed.py stores them) skip HuBERT entirely:
``quantize_features`` / ``encode_features``.

By default inference only: ``forward`` has the reference's eval semantics in either mode (loss 0, Dropout the identity, no EMA
codebook update).  ``autograd=True`` (FSQ heads) makes the head trainable as train_v2.train_step trains it: under grad mode
``forward`` / ``quantize_features`` / ``forward_features`` run the training forward (edtts_sem_encode_train) and ``backward()`` the
backward kernels (edtts_sem_backward), with FSQ's straight-through estimator; ``train_dropout=True`` adds proj's ``nn.Dropout`` with
masks from the library's Philox stream.  ``autograd=True, train_vq=True`` does the same for a VQ head as
train.py trains it: VectorQuantizer's codebook and commitment losses, straight-through estimator, EMA codebook update and dead-code
reset (edtts_sem_vq_*).  fp32 only: bf16 / autocast training is not built.  Weights are packed for the kernels
on first use and re-packed when a parameter changes.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import torch
import torch.nn as nn

from . import native
from ._cache import PackedBlob


# (byte-count query, pack call) of a head's inference blob and of its training-only blob (transposed matrices for the backward), FSQ / VQ
_SEM = (native.sem_packed_bytes, native.sem_pack)
_SEM_TRAIN = (native.sem_train_packed_bytes, native.sem_train_pack)
_SEM_VQ_TRAIN = (native.sem_vq_train_packed_bytes, native.sem_vq_train_pack)


def _stats(counts: torch.Tensor):
    return native.sem_stats(counts)


def _flat3(z: torch.Tensor, width: int, name: str) -> torch.Tensor:
    if z.shape[-1] != width:
        raise ValueError(f"{name}: expected last dimension {width}, got {list(z.shape)}")
    return z.float().reshape(1, -1, width)


def _train_input(h: torch.Tensor, lengths: Optional[torch.Tensor]):
    """(x, B, T): a training forward's input as the kernels take it -- detached, fp32, aligned, rows past the lengths zeroed."""
    x = native._aligned(h.detach().float())
    B, T = x.shape[0], x.shape[1]
    if lengths is not None and B * T:  # the weight-gradient products multiply the rows past the lengths by zeros: make them finite
        x = x.masked_fill((torch.arange(T, device=x.device)[None, :] >= lengths.clamp(1, T)[:, None])[..., None], 0.0)
    return x, B, T


class _SemGrad(torch.autograd.Function):
    """(z_q, idx, counts) of a head on the training forward (edtts_sem_encode_train); backward through edtts_sem_backward.  The tape
    is a tensor of this call's own, saved in ctx; ``drop`` (None or this call's (p, seed)) lives in ctx too, so the backward
    regenerates the mask of ITS forward.  ``owner``: the module whose ``_slots()`` / ``_pack`` / ``_tpack`` describe the head."""

    @staticmethod
    def forward(ctx, owner, dims, lengths, drop, h, *params):
        slots = owner._slots()
        blob = owner._pack.get(dims, slots, trainable=True)  # (under graph capture: packed inside the capture, _cache.capture_scope)
        tblob = owner._tpack.get(dims, slots, trainable=True)
        x, B, T = _train_input(h, lengths)
        tape = torch.empty(native.sem_train_tape_bytes(dims, B, T), dtype=torch.uint8, device=x.device)
        idx, zq, counts = native.sem_encode_train(dims, blob, x, tape, lengths, True, drop)
        ctx.owner, ctx.dims, ctx.lengths, ctx.drop, ctx.sig = owner, dims, lengths, drop, (owner._pack.sig, owner._tpack.sig)
        ctx.x = x
        ctx.save_for_backward(tape, *params)
        ctx.mark_non_differentiable(idx, counts)
        return zq, idx, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_zq, _d_idx, _d_counts):
        owner, dims = ctx.owner, ctx.dims
        tape, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        slots = owner._slots()
        blob = owner._pack.get(dims, slots, trainable=True)
        tblob = owner._tpack.get(dims, slots, trainable=True)
        if (owner._pack.sig, owner._tpack.sig) != ctx.sig:
            raise RuntimeError(f"{type(owner).__name__}: a parameter was modified between this forward and its backward")
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[5:])]
        d_z = torch.empty_like(ctx.x) if dims.in_dim == 0 and ctx.needs_input_grad[4] else None
        native.sem_backward(dims, blob, tblob, tape, ctx.x, ctx.lengths, native._aligned(d_zq.float()), grads, d_z, ctx.drop)
        return (None, None, None, None, d_z, *grads)


class _VQGrad(torch.autograd.Function):
    """(z_q, vq_loss, idx, counts) of a VQ head on the training forward (edtts_sem_vq_encode_train), then -- module in training mode,
    decay > 0 -- VectorQuantizer's EMA update and dead-code reset; backward through edtts_sem_vq_backward.  The reference's order
    (models/vq.py:86-93): the loss and both gradients refer to the codebook the forward was given, which the EMA update has
    overwritten by the time the backward runs, so the tape carries r = c - z and the backward reads nothing of the codebook.
    ``owner``: the module whose ``_slots()`` / ``_pack`` / ``_tpack`` describe the head; ``vq``: its VectorQuantizer."""

    @staticmethod
    def forward(ctx, owner, vq, dims, lengths, drop, h, *params):
        slots = owner._slots()
        blob = owner._pack.get(dims, slots)
        tblob = owner._tpack.get(dims, slots)
        x, B, T = _train_input(h, lengths)
        training = bool(vq.training)
        commit = float(vq.commit)
        tape = torch.empty(native.sem_vq_tape_bytes(dims, B, T), dtype=torch.uint8, device=x.device)
        idx, zq, counts, loss = native.sem_vq_encode_train(dims, blob, x, tape, lengths, training, commit, drop)
        # the versions as the forward saw them: the EMA's own write (no version moves, the caches are only marked stale) must not
        # look like a modified parameter to the backward
        ctx.owner, ctx.dims, ctx.lengths, ctx.drop, ctx.sig = owner, dims, lengths, drop, PackedBlob.signature(dims, slots)
        ctx.blob, ctx.tblob, ctx.commit, ctx.training = blob, tblob, commit, training
        ctx.x = x
        if training and vq.decay > 0:
            z = x  # without a proj the input itself; with one, where the library says the tape holds z
            if dims.in_dim:
                off, n = native.sem_train_region(dims, B, T, "tape.z")
                z = tape[off:off + n].view(torch.float32).view(B, T, dims.semantic_dim)
            vq._ema_update(dims, idx, z, lengths, counts)
            owner._pack.invalidate()
            vq._pack.invalidate()
        ctx.save_for_backward(tape, idx, *params)
        ctx.mark_non_differentiable(idx, counts)
        ctx.set_materialize_grads(False)
        return zq, loss, idx, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_zq, d_loss, _d_idx, _d_counts):
        owner, dims = ctx.owner, ctx.dims
        tape, idx, params = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        if PackedBlob.signature(dims, owner._slots()) != ctx.sig:
            raise RuntimeError(f"{type(owner).__name__}: a parameter was modified between this forward and its backward")
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[6:])]
        d_z = torch.empty_like(ctx.x) if dims.in_dim == 0 and ctx.needs_input_grad[5] else None
        if d_zq is not None:
            d_zq = native._aligned(d_zq.float())
        if d_loss is not None:
            d_loss = d_loss.float().reshape(()).contiguous() if ctx.training else None  # (eval: vq_loss is the constant 0)
        # (the proj regions of the forward's blobs are what the backward reads: the checked versions are the ones they were packed from)
        native.sem_vq_backward(dims, ctx.blob, ctx.tblob, tape, ctx.x, idx, ctx.lengths, d_zq, d_loss, ctx.commit, grads, d_z, ctx.drop)
        return (None, None, None, None, None, d_z, *grads)


class FSQ(nn.Module):
    """Finite Scalar Quantization (reference models/fsq.py:FSQ): state-dict keys ``_levels`` and ``_basis``.  forward(z [..., dim]) ->
    (z_q, indices) on the kernels: the head kernel runs with identity projections, which MFMA applies exactly (one product by 1,
    the rest by 0)."""

    def __init__(self, levels: List[int]):
        super().__init__()
        self.levels = [int(v) for v in levels]
        self.dim = len(self.levels)
        self.register_buffer("_levels", torch.tensor(self.levels, dtype=torch.int32))
        self.register_buffer("_basis", torch.cumprod(torch.tensor([1] + self.levels[:-1], dtype=torch.int64), dim=0))
        self.codebook_size = 1
        for v in self.levels:
            self.codebook_size *= v
        self._pack = PackedBlob(*_SEM)
        self._eye = {}

    @property
    def num_codes(self) -> int:
        return self.codebook_size

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        lv = state_dict.get(prefix + "_levels")
        if lv is not None and lv.numel() == self.dim:
            self.levels = [int(v) for v in lv.tolist()]
            self.codebook_size = 1
            for v in self.levels:
                self.codebook_size *= v
        super()._load_from_state_dict(state_dict, prefix, *args, **kw)

    def _dims(self) -> native.EdttsSemDims:
        return native.sem_dims(0, 16, self.levels)

    def _identity(self, dev) -> List[torch.Tensor]:
        key = str(dev)
        if key not in self._eye:
            D = self.dim
            if not 1 <= D <= 16:
                raise native.EdttsError(f"FSQ: {D} levels, the kernels take 1..16")
            eye = torch.eye(16, dtype=torch.float32)
            self._eye[key] = [t.to(dev) for t in (eye[:D].contiguous(), torch.zeros(D), eye[:, :D].contiguous(), torch.zeros(16))]
        return self._eye[key]

    def _run(self, z: torch.Tensor, want_zq: bool):
        shape = z.shape[:-1]
        flat = _flat3(z.float(), self.dim, "FSQ input")
        pad = torch.zeros((1, flat.shape[1], 16), dtype=torch.float32, device=z.device)
        pad[..., : self.dim] = flat
        dims = self._dims()
        blob = self._pack.get(dims, self._identity(z.device))
        idx, _, zq, _ = native.sem_encode(dims, blob, pad, want_zq=want_zq, want_counts=False)
        return (zq[0, :, : self.dim].reshape(*shape, self.dim) if want_zq else None), idx.reshape(shape)

    def forward(self, z: torch.Tensor):
        return self._run(z, True)

    def encode(self, z: torch.Tensor) -> torch.Tensor:
        return self._run(z, False)[1]

    def indices_to_codes(self, indices: torch.Tensor) -> torch.Tensor:
        """Codes in [-1, 1] from flat indices, as the reference computes them (its last level is the least significant digit)."""
        dims = self._dims()
        blob = self._pack.get(dims, self._identity(indices.device))
        return native.sem_decode(dims, blob, indices.to(torch.int64))[..., : self.dim]

    decode = indices_to_codes


class FSQEncoder(nn.Module):
    """proj_down -> FSQ -> proj_up (reference models/fsq.py:FSQEncoder); keys ``fsq._levels``, ``fsq._basis``, ``proj_down.*``,
    ``proj_up.*``."""

    def __init__(self, input_dim: int, levels: List[int] = (8, 6, 5, 5, 5), autograd: bool = False):
        """``autograd``: False (default) -- inference only, as before.  True -- under grad mode ``forward`` is differentiable with
        respect to ``proj_down``, ``proj_up`` and the input ``z`` (FSQ's straight-through estimator)."""
        super().__init__()
        self.autograd = bool(autograd)
        self.fsq = FSQ(list(levels))
        self.fsq_dim = len(levels)
        self.proj_down = nn.Linear(input_dim, self.fsq_dim)
        self.proj_up = nn.Linear(self.fsq_dim, input_dim)
        self._pack = PackedBlob(*_SEM)
        self._tpack = PackedBlob(*_SEM_TRAIN)

    @property
    def codebook_size(self) -> int:
        return self.fsq.codebook_size

    @property
    def num_codes(self) -> int:
        return self.fsq.codebook_size

    def _dims(self, in_dim: int = 0) -> native.EdttsSemDims:
        return native.sem_dims(in_dim, self.proj_up.out_features, self.fsq.levels)

    def _slots(self) -> List[torch.Tensor]:
        return [self.proj_down.weight, self.proj_down.bias, self.proj_up.weight, self.proj_up.bias]

    def _quantize(self, z: torch.Tensor, want_zq: bool, want_counts: bool):
        shape = z.shape[:-1]
        dims = self._dims()
        blob = self._pack.get(dims, self._slots())
        idx, _, zq, counts = native.sem_encode(dims, blob, _flat3(z, dims.semantic_dim, "FSQEncoder input"), want_zq=want_zq,
                                               want_counts=want_counts)
        return (None if zq is None else zq.reshape(*shape, -1)), idx.reshape(shape), counts

    def forward(self, z: torch.Tensor):
        """(z_q, indices, loss = 0, perplexity, used), as FSQEncoder.forward returns them.  With ``autograd=True`` and under grad
        mode z_q carries the graph."""
        if self.autograd and torch.is_grad_enabled():
            shape = z.shape[:-1]
            dims = self._dims()
            zq, idx, counts = _SemGrad.apply(self, dims, None, None, _flat3(z, dims.semantic_dim, "FSQEncoder input"), *self._slots())
            zq, idx = zq.reshape(*shape, -1), idx.reshape(shape)
        else:
            with torch.no_grad():
                zq, idx, counts = self._quantize(z, True, True)
        with torch.no_grad():
            ppl, used = _stats(counts)
        return zq, idx, torch.zeros((), device=z.device), ppl, used

    @torch.no_grad()
    def encode(self, z: torch.Tensor) -> torch.Tensor:
        return self._quantize(z, False, False)[1]

    @torch.no_grad()
    def decode(self, indices: torch.Tensor) -> torch.Tensor:
        dims = self._dims()
        return native.sem_decode(dims, self._pack.get(dims, self._slots()), indices.to(torch.int64))


class VectorQuantizer(nn.Module):
    """Nearest-code quantizer (reference models/vq.py:VectorQuantizer); keys ``codebook.weight``, ``ema_cluster_size``, ``ema_w``,
    ``update_count``.  By default inference only: the loss is 0 and the EMA codebook update is not run."""

    def __init__(self, dim: int, codebook_size: int, commit: float = 0.25, decay: float = 0.99, epsilon: float = 1e-5,
                 reset_unused_every: int = 100, autograd: bool = False):
        """``autograd``: False (default) -- inference only, as before.  True -- under grad mode ``forward`` is the reference's
        training forward: z_q carries the straight-through gradient to ``z``; in training mode vq_loss =
        codebook loss + commit x commitment loss carries the graph to ``z`` and ``codebook.weight``, and (decay > 0) the EMA update
        of ``ema_cluster_size`` / ``ema_w`` / ``codebook.weight`` and the dead-code reset run; in eval mode vq_loss is 0 and no
        buffer changes.  The reset's permutation is drawn on the host, ``torch.randperm(N, generator=self.reset_generator)`` (a CPU
        ``torch.Generator``; None: torch's default one), only on a reset step with a dead code."""
        super().__init__()
        self.dim = dim
        self.codebook_size = codebook_size
        self.commit, self.decay, self.epsilon, self.reset_unused_every = commit, decay, epsilon, reset_unused_every
        self.autograd = bool(autograd)
        self.codebook = nn.Embedding(codebook_size, dim)
        nn.init.normal_(self.codebook.weight, mean=0.0, std=1.0)
        self.register_buffer("ema_cluster_size", torch.ones(codebook_size))
        self.register_buffer("ema_w", self.codebook.weight.detach().clone())
        self.register_buffer("update_count", torch.tensor(0))
        self._pack = PackedBlob(*_SEM)
        self._tpack = PackedBlob(*_SEM_VQ_TRAIN)
        self.reset_generator: Optional[torch.Generator] = None
        self._count_host: Optional[int] = None  # host mirror of update_count: a step that does not reset never synchronises
        self._count_sig = None

    @property
    def num_codes(self) -> int:
        return self.codebook_size

    def _dims(self, in_dim: int = 0) -> native.EdttsSemDims:
        return native.sem_dims(in_dim, self.dim, codebook_size=self.codebook_size)

    def _slots(self) -> List[torch.Tensor]:
        return [self.codebook.weight]

    def _quantize(self, z: torch.Tensor, want_zq: bool, want_counts: bool):
        shape = z.shape[:-1]
        dims = self._dims()
        blob = self._pack.get(dims, self._slots())
        idx, _, zq, counts = native.sem_encode(dims, blob, _flat3(z, self.dim, "VectorQuantizer input"), want_zq=want_zq,
                                               want_counts=want_counts)
        return (None if zq is None else zq.reshape(*shape, -1)), idx.reshape(shape), counts

    # ------------------------------------------------------------------------------------------ training
    def _bump_count(self) -> int:
        """update_count += 1 on the device and in the host mirror (re-read when the buffer was loaded or moved); returns it."""
        u = self.update_count
        sig = (u.data_ptr(), u._version, u.device)
        if self._count_host is None or sig != self._count_sig:
            self._count_host = int(u)
        u += 1
        self._count_host += 1
        self._count_sig = (u.data_ptr(), u._version, u.device)
        return self._count_host

    @torch.no_grad()
    def _ema_update(self, dims, idx: torch.Tensor, z: torch.Tensor, lengths, counts: torch.Tensor) -> None:
        """VectorQuantizer._ema_update (models/vq.py:109-145) after a training forward: idx [B, T], z [B, T, dim] fp32, counts the
        usage of this batch.  The EMA lines run in one kernel chain on the buffers' and the codebook's storage (no version moves: the
        caller marks the pack caches stale); the reset is torch plumbing on the reset steps only."""
        w = self.codebook.weight
        for t, name in ((self.ema_cluster_size, "ema_cluster_size"), (self.ema_w, "ema_w"), (w, "codebook.weight")):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != idx.device:
                raise native.EdttsError(f"VectorQuantizer: {name} must be a contiguous fp32 tensor on {idx.device}")
        native.sem_vq_ema_update(dims, idx, z, lengths, counts, self.decay, self.epsilon, self.ema_cluster_size, self.ema_w, w.data)
        count = self._bump_count()
        if not (self.reset_unused_every > 0 and count % self.reset_unused_every == 0):
            return
        dead = self.ema_cluster_size < 1.0
        num_dead = int(dead.sum())  # (a host synchronisation on the reset steps, as the reference's .item())
        B, T = idx.shape
        if lengths is None:
            rows_of = None
            n_valid = B * T
        else:
            valid = torch.arange(T, device=idx.device)[None, :] < lengths.clamp(1, max(T, 1))[:, None]
            rows_of = valid.reshape(-1).nonzero(as_tuple=True)[0]
            n_valid = int(rows_of.numel())
        if num_dead == 0 or n_valid == 0:
            return
        num_replace = min(num_dead, n_valid)
        pick = torch.randperm(n_valid, generator=self.reset_generator)[:num_replace].to(idx.device)
        rows = pick if rows_of is None else rows_of[pick]
        new = z.reshape(-1, self.dim).index_select(0, rows)
        dead_idx = dead.nonzero(as_tuple=True)[0][:num_replace]
        w.data.index_copy_(0, dead_idx, new)
        self.ema_w.index_copy_(0, dead_idx, new)
        self.ema_cluster_size.index_fill_(0, dead_idx, 1.0)

    def forward(self, z: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """(z_q, idx, vq_loss, perplexity, used), as VectorQuantizer.forward returns them.  Without ``autograd`` or outside grad
        mode: eval semantics (vq_loss = 0).  ``lengths`` (int64 [B], z [B, T, dim]): frames t >= lengths[b] are not read."""
        if self.autograd and torch.is_grad_enabled():
            shape = z.shape[:-1]
            dims = self._dims()
            if lengths is not None:
                if z.dim() != 3:
                    raise ValueError(f"VectorQuantizer: lengths need z [B, T, {self.dim}], got {list(z.shape)}")
                if z.shape[-1] != self.dim:
                    raise ValueError(f"VectorQuantizer input: expected last dimension {self.dim}, got {list(z.shape)}")
                zz = z.float()
                lengths = native.lengths(lengths, z.shape[0], max(z.shape[1], 1), z.device, "lengths")
            else:
                zz = _flat3(z, self.dim, "VectorQuantizer input")
            zq, loss, idx, counts = _VQGrad.apply(self, self, dims, lengths, None, zz, *self._slots())
            zq, idx = zq.reshape(*shape, -1), idx.reshape(shape)
        else:
            with torch.no_grad():
                if lengths is not None:
                    dims = self._dims()
                    n = native.lengths(lengths, z.shape[0], max(z.shape[1], 1), z.device, "lengths")
                    idx, _, zq, counts = native.sem_encode(dims, self._pack.get(dims, self._slots()), z.float(), n)
                else:
                    zq, idx, counts = self._quantize(z, True, True)
            loss = torch.zeros((), device=z.device)
        with torch.no_grad():
            ppl, used = _stats(counts)
        return zq, idx, loss, ppl, used

    @torch.no_grad()
    def encode(self, z: torch.Tensor) -> torch.Tensor:
        return self._quantize(z, False, False)[1]

    @torch.no_grad()
    def decode(self, idx: torch.Tensor) -> torch.Tensor:
        dims = self._dims()
        return native.sem_decode(dims, self._pack.get(dims, self._slots()), idx.to(torch.int64))


class _Proj(nn.Sequential):
    """proj of the reference: Linear, GELU, LayerNorm, Linear (models/encoder.py:40-45) or with a Dropout before the last Linear
    (train_v2.py:54-60, inference_pipeline.py:29-35).  Loading a state dict of either layout switches to that layout."""

    def __init__(self, in_dim: int, dim: int, dropout: Optional[float] = None):
        layers = [nn.Linear(in_dim, dim), nn.GELU(), nn.LayerNorm(dim)]
        if dropout is not None:
            layers.append(nn.Dropout(dropout))
        super().__init__(*layers, nn.Linear(dim, dim))

    @property
    def final(self) -> nn.Linear:
        return self[len(self) - 1]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        has4, has3 = (prefix + "4.weight") in state_dict, (prefix + "3.weight") in state_dict
        if has4 != has3 and has4 != (len(self) == 5):
            lin = self.final
            mods = [self[0], self[1], self[2]] + ([nn.Dropout(0.0)] if has4 else []) + [lin]
            self._modules = OrderedDict((str(i), m) for i, m in enumerate(mods))
        super()._load_from_state_dict(state_dict, prefix, *args, **kw)


def _missing_hubert(hubert_id: str, err: Exception) -> RuntimeError:
    return RuntimeError(
        f"SemanticEncoder: no HuBERT module was given and {hubert_id!r} is not in the local Hugging Face cache ({err}).  This package "
        "never downloads: put the model in the cache beforehand, pass hubert=<module>, or use quantize_features / encode_features "
        "on precomputed features.")


class SemanticEncoder(nn.Module):
    """HuBERT features -> proj -> FSQ / VQ (reference models/encoder.py:SemanticEncoder), with the head on the kernels.

    ``hubert``: a module called as ``hubert(wav, output_hidden_states=True)`` returning ``.hidden_states``; the head reads
    ``hidden_states[cfg.hubert_layer]``.  None: nothing is loaded here; the first waveform call loads
    ``HubertModel.from_pretrained(cfg.hubert_id, local_files_only=True)`` and raises a RuntimeError if it is not cached."""

    def __init__(self, cfg, hubert: Optional[nn.Module] = None, *, in_dim: int = 768, proj_dropout: bool = False,
                 autograd: bool = False, train_dropout: bool = False, train_vq: bool = False):
        """``autograd``: False (default) -- inference only, as before.  True -- ``forward``, ``quantize_features`` and
        ``forward_features`` under grad mode return a z_q that carries the graph to proj and the quantizer's projections.  No
        gradient goes into HuBERT (the reference detaches its features).  On a VQ config ``autograd=True`` alone raises a
        ValueError: the VQ path is asked for by name with ``train_vq=True``.
        ``train_vq``: False (default).  True (needs ``autograd=True`` and a VQ config, ``cfg.use_fsq`` false) -- the head trains as
        train.py trains it: in training mode ``forward`` / ``forward_features`` return VectorQuantizer's vq_loss (codebook loss +
        ``cfg.vq_commit`` x commitment loss) with the graph to proj and ``vq.codebook.weight``, and every such call runs the EMA
        codebook update and, every ``vq.reset_unused_every`` updates, the dead-code reset (its permutation from
        ``self.vq.reset_generator``); in eval mode vq_loss is 0 and no buffer changes.  fp32 only.
        ``train_dropout``: False (default) -- a differentiable call in training mode with the Dropout layout and ``p > 0`` raises.
        True (needs ``autograd=True`` and the Dropout layout) -- that call applies ``proj[3]`` with the library's Philox masks: each
        draws a 63-bit seed on the host from ``self.dropout_generator`` (a CPU ``torch.Generator``; None: torch's default one),
        keeps it for its own backward and shows it as ``self.last_dropout_seed``, as EdgeDiffusionDecoder does.  With
        ``self.dropout_keys = (key_stream, first_slot)`` the forward takes a slot of the stream instead -- ``first_slot`` for this
        module's first forward since the stream's last ``advance()``, then the next (a key in device memory, DESIGN.md section
        32; FSQ head only) -- and ``last_dropout_seed`` is None."""
        super().__init__()
        self.autograd = bool(autograd)
        self.train_dropout = bool(train_dropout)
        self.train_vq = bool(train_vq)
        is_fsq = bool(getattr(cfg, "use_fsq", False))
        if self.train_vq and not self.autograd:
            raise ValueError("train_vq=True needs autograd=True (the VQ losses, EMA update and dead-code reset belong to the training forward)")
        if self.train_vq and is_fsq:
            raise ValueError("train_vq=True needs a VQ config (cfg.use_fsq is set: an FSQ head trains with autograd=True alone)")
        if self.autograd and not is_fsq and not self.train_vq:
            raise ValueError("autograd=True alone covers the FSQ quantizer (cfg.use_fsq): the VQ path -- VectorQuantizer in training mode "
                             "with its codebook loss, commitment loss, EMA update and dead-code reset -- is switched on with train_vq=True")
        if self.train_dropout and not self.autograd:
            raise ValueError("train_dropout=True needs autograd=True (dropout belongs to the training forward and its backward)")
        if self.train_dropout and not proj_dropout:
            raise ValueError("train_dropout=True needs the Dropout layout of proj (proj_dropout=True: Linear, GELU, LayerNorm, Dropout, "
                             "Linear as train_v2.py builds it)")
        if self.train_dropout:
            p = float(getattr(cfg, "dropout", 0.0))
            if not (0.0 <= p < 1.0) or round(p * 65536.0) > 65535:
                raise ValueError(f"train_dropout=True: cfg.dropout={p} is outside [0, 1) (the mask contract needs round(p * 65536) <= 65535)")
        self.dropout_generator: Optional[torch.Generator] = None
        self.last_dropout_seed: Optional[int] = None
        self.dropout_keys = None  # (KeyStream, first slot): the dropout key from device memory instead of a host draw
        self.cfg = cfg
        self.hubert = hubert
        if hubert is not None:
            self._check_native(hubert, cfg)
            self._freeze(hubert)
        self.proj = _Proj(in_dim, cfg.semantic_dim, getattr(cfg, "dropout", 0.0) if proj_dropout else None)
        if getattr(cfg, "use_fsq", False):
            self.vq = FSQEncoder(cfg.semantic_dim, cfg.fsq_levels, autograd=self.autograd)
        else:
            self.vq = VectorQuantizer(cfg.semantic_dim, cfg.codebook_size, commit=getattr(cfg, "vq_commit", 0.25), autograd=self.train_vq)
        self._pack = PackedBlob(*_SEM)
        self._tpack = PackedBlob(*(_SEM_TRAIN if is_fsq else _SEM_VQ_TRAIN))

    @property
    def codebook_size(self) -> int:
        return self.vq.codebook_size

    def get_trainable_params(self) -> list:
        """proj and quantizer parameters (reference models/encoder.py:129-131, train_v2.py:80-81): what the trainer's optimiser gets
        next to ``decoder.parameters()``.  HuBERT is frozen."""
        return list(self.proj.parameters()) + list(self.vq.parameters())

    @staticmethod
    def _check_native(hubert: nn.Module, cfg) -> None:
        from .hubert import NativeHubert
        if isinstance(hubert, NativeHubert) and hubert.num_layers != cfg.hubert_layer:
            raise ValueError(f"SemanticEncoder: the NativeHubert backbone runs {hubert.num_layers} layers, the head reads "
                             f"hidden_states[cfg.hubert_layer={cfg.hubert_layer}]")

    @staticmethod
    def _freeze(m: nn.Module) -> None:
        m.eval()
        for p in m.parameters():
            p.requires_grad = False

    # ------------------------------------------------------------------------------------------ loading
    @classmethod
    def from_checkpoint(cls, ckpt_or_path, cfg=None, hubert: Optional[nn.Module] = None, device=None) -> "SemanticEncoder":
        """Build the head from a reference checkpoint (a dict or a path): ``encoder_proj`` + ``encoder_vq`` (train.py:291-297),
        ``encoder_proj`` + ``encoder_fsq`` (train_v2.py:335-341), or a full ``encoder`` state dict (train.py:195).  The quantizer
        kind, its levels / codebook size, semantic_dim, the HuBERT width and the proj layout come from the tensors.  In a full
        ``encoder`` dict the ``hubert.*`` keys are loaded into ``hubert`` when one is given and ignored otherwise."""
        from .config import CFG
        ck = ckpt_or_path
        if isinstance(ck, (str, bytes)) or hasattr(ck, "__fspath__"):
            ck = torch.load(ck, map_location="cpu", weights_only=False)
        if "encoder_proj" in ck:
            proj_sd = dict(ck["encoder_proj"])
            q_sd = ck.get("encoder_fsq", ck.get("encoder_vq"))
            if q_sd is None:
                raise KeyError("checkpoint has encoder_proj but neither encoder_fsq nor encoder_vq")
            q_sd, hub_sd = dict(q_sd), {}
        else:
            sd = ck["encoder"] if "encoder" in ck else ck
            proj_sd = {k[len("proj."):]: v for k, v in sd.items() if k.startswith("proj.")}
            q_sd = {k[len("vq."):]: v for k, v in sd.items() if k.startswith("vq.")}
            hub_sd = {k[len("hubert."):]: v for k, v in sd.items() if k.startswith("hubert.")}
            if not proj_sd or not q_sd:
                raise KeyError("no encoder weights found: expected encoder_proj + encoder_fsq / encoder_vq, or an encoder state dict")
        if cfg is None:
            stored = ck.get("cfg") if isinstance(ck, dict) else None
            if isinstance(stored, dict):
                cfg = CFG.from_dict(dict(stored))
            elif stored is not None:
                cfg = CFG.from_dict({k: getattr(stored, k) for k in CFG.__dataclass_fields__ if hasattr(stored, k) and k != "phase"})
            else:
                cfg = CFG(device="cpu")
        w0 = proj_sd["0.weight"]
        cfg.semantic_dim = int(w0.shape[0])
        if "fsq._levels" in q_sd:
            cfg.use_fsq = True
            cfg.fsq_levels = [int(v) for v in q_sd["fsq._levels"].tolist()]
        elif "codebook.weight" in q_sd:
            cfg.use_fsq = False
            cfg.codebook_size = int(q_sd["codebook.weight"].shape[0])
        else:
            raise KeyError("quantizer state dict has neither fsq._levels (FSQ) nor codebook.weight (VQ)")
        enc = cls(cfg, hubert, in_dim=int(w0.shape[1]), proj_dropout="4.weight" in proj_sd)
        enc.proj.load_state_dict(proj_sd)
        enc.vq.load_state_dict(q_sd)
        if hubert is not None and hub_sd:
            hubert.load_state_dict(hub_sd)
        if device is not None:
            enc = enc.to(device)
        return enc.eval()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if self.hubert is None:  # a full encoder dict carries the backbone: without a HuBERT module its keys are ignored
            hub = [k for k in state_dict if k.startswith(prefix + "hubert.")]
            for k in hub:
                if k in unexpected_keys:
                    unexpected_keys.remove(k)

    # ------------------------------------------------------------------------------------------ HuBERT
    def _backbone(self) -> nn.Module:
        if self.hubert is None:
            try:
                from transformers import HubertModel
            except ImportError as e:
                raise _missing_hubert(self.cfg.hubert_id, e) from e
            try:
                m = HubertModel.from_pretrained(self.cfg.hubert_id, local_files_only=True)
            except OSError as e:
                raise _missing_hubert(self.cfg.hubert_id, e) from e
            self._freeze(m)
            self.hubert = m.to(self.proj[0].weight.device)
        return self.hubert

    def _native(self):
        from .hubert import NativeHubert
        if isinstance(self.hubert, NativeHubert):
            self._check_native(self.hubert, self.cfg)
            return self.hubert
        return None

    @torch.no_grad()
    def extract_hubert(self, wav_16k: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HuBERT features [B, T_feat, 768] of a 16 kHz waveform [B, T_audio]: hidden_states[cfg.hubert_layer].  ``lengths`` (int64
        [B] sample counts) needs a NativeHubert backbone: row b is then the features of wav[b, :lengths[b]] alone, zero past them."""
        nat = self._native()
        if nat is not None:
            return nat(wav_16k, lengths)
        if lengths is not None:
            raise ValueError("SemanticEncoder: per-utterance lengths need a NativeHubert backbone (a torch HuBERT normalises over the "
                             "padded batch)")
        out = self._backbone()(wav_16k, output_hidden_states=True)
        return out.hidden_states[self.cfg.hubert_layer].float()

    def _features(self, wav_16k: torch.Tensor, lengths):
        """(features, their per-utterance frame counts on the device or None)"""
        h = self.extract_hubert(wav_16k, lengths)
        if lengths is None:
            return h, None
        n = native.lengths(lengths, wav_16k.shape[0], wav_16k.shape[1], h.device, "lengths")
        return h, self.hubert.frames_of(n, wav_16k.shape[1])

    # ------------------------------------------------------------------------------------------ the head
    def _dims(self) -> native.EdttsSemDims:
        return self.vq._dims(self.proj[0].in_features)

    def _slots(self) -> List[torch.Tensor]:
        p = self.proj
        return [p[0].weight, p[0].bias, p[2].weight, p[2].bias, p.final.weight, p.final.bias] + self.vq._slots()

    def _head(self, h: torch.Tensor, lengths, want_zq: bool, want_counts: bool, want_z: bool = False):
        if h.dim() != 3:
            raise ValueError(f"features: expected [B, T_feat, {self.proj[0].in_features}], got {list(h.shape)}")
        dims = self._dims()
        blob = self._pack.get(dims, self._slots())
        B, T = h.shape[0], h.shape[1]
        n = native.lengths(lengths, B, max(T, 1), h.device, "lengths")
        return native.sem_encode(dims, blob, h.float(), n, want_z=want_z, want_zq=want_zq, want_counts=want_counts)

    def _head_autograd(self, h: torch.Tensor, lengths):
        """(z_q with the graph, idx, counts, vq_loss -- None for FSQ) of a differentiable call."""
        if h.dim() != 3:
            raise ValueError(f"features: expected [B, T_feat, {self.proj[0].in_features}], got {list(h.shape)}")
        drop = None
        layer = self.proj[3] if len(self.proj) == 5 else None
        if self.training and layer is not None and layer.p > 0:
            if not self.train_dropout:
                raise ValueError(f"autograd=True: proj has a Dropout with p={layer.p} and the encoder is in training mode (the reference "
                                 "drops there), but train_dropout is off: construct with train_dropout=True, or set proj[3].p = 0 or "
                                 "call .eval()")
            if self.dropout_keys is not None:
                if self.train_vq:
                    raise ValueError("dropout_keys: the VQ head's training forward takes host seeds only (train_vq=True stays outside "
                                     "a captured step)")
                drop = native.DropKey(float(layer.p), self.dropout_keys[0].take(self, self.dropout_keys[1]))
                self.last_dropout_seed = None
            else:
                # (a host draw from a CPU generator: no device work, no synchronisation)
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=self.dropout_generator).item())
                drop = (float(layer.p), seed)
                self.last_dropout_seed = seed
        n = native.lengths(lengths, h.shape[0], max(h.shape[1], 1), h.device, "lengths")
        if self.train_vq:
            zq, loss, idx, counts = _VQGrad.apply(self, self.vq, self._dims(), n, drop, h.detach(), *self._slots())
            return zq, idx, counts, loss
        return (*_SemGrad.apply(self, self._dims(), n, drop, h.detach(), *self._slots()), None)

    def _differentiable(self) -> bool:
        return self.autograd and torch.is_grad_enabled()

    def _quantize_loss(self, h: torch.Tensor, lengths):
        loss = None
        if self._differentiable():
            zq, idx, counts, loss = self._head_autograd(h, lengths)
        else:
            with torch.no_grad():
                idx, _, zq, counts = self._head(h, lengths, True, True)
        with torch.no_grad():
            ppl, used = _stats(counts)
        return zq, idx, (torch.zeros((), device=zq.device) if loss is None else loss), ppl, used

    def quantize_features(self, h: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """Precomputed HuBERT features h [B, T_feat, 768] -> (z_q [B, T_feat, semantic_dim], idx [B, T_feat], perplexity, used).
        ``lengths`` (int64 [B]): frames t >= lengths[b] are not read, get idx 0 and z_q 0, and are not counted.  With
        ``autograd=True`` and under grad mode z_q carries the graph (the features themselves get no gradient); with ``train_vq=True``
        the call is a training forward like ``forward_features`` (EMA update included), only its vq_loss is not returned."""
        zq, idx, _, ppl, used = self._quantize_loss(h, lengths)
        return zq, idx, ppl, used

    def forward_features(self, h: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """``forward`` from precomputed HuBERT features: (z_q, idx, vq_loss, perplexity, used); vq_loss is 0 except for a
        ``train_vq=True`` head in training mode under grad."""
        return self._quantize_loss(h, lengths)

    @torch.no_grad()
    def encode_features(self, h: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Token ids [B, T_feat] of precomputed HuBERT features (see quantize_features)."""
        return self._head(h, lengths, False, False)[0]

    def forward(self, wav_16k: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """(z_q, idx, vq_loss, perplexity, used) of a 16 kHz waveform [B, T_audio], as the reference returns them (vq_loss: see
        ``forward_features``).  ``lengths``
        (sample counts, NativeHubert backbone only): the head then takes each utterance's own frame count.  HuBERT runs without
        grad in every mode; see ``quantize_features`` for ``autograd=True``."""
        with torch.no_grad():
            feats = self._features(wav_16k, lengths)
        return self.forward_features(*feats)

    @torch.no_grad()
    def encode(self, wav_16k: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Token ids [B, T_feat] of a 16 kHz waveform (``lengths`` as in forward)."""
        return self.encode_features(*self._features(wav_16k, lengths))

    @torch.no_grad()
    def decode_tokens(self, idx: torch.Tensor) -> torch.Tensor:
        """Token ids -> continuous features [..., semantic_dim] (the quantizer's decode)."""
        return self.vq.decode(idx)
