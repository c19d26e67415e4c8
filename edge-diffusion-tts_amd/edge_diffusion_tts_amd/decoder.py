"""EdgeDiffusionDecoder -- API mirror of /root/reference/edge_diffusion_tts/models/decoder.py:14-109 on MI355X.

The module owns parameters and buffers under the reference's state-dict key names, so
``load_state_dict(reference_decoder.state_dict())`` works, but it has no sub-module forward code: ``forward`` hands
device pointers to the C ABI (include/edtts.h, edtts_decoder_forward) where the whole network runs as hand-written
gfx950 kernels.  By default inference only (the reference path this replaces runs under ``torch.no_grad``, inference.py:23);
dropout is the identity as in ``decoder.eval()``.  ``autograd=True`` (generic fp32 kernels) adds the backward the reference's
trainers need (train_v2.py train_step, training/consistency.py): DESIGN.md section 19.  ``train_dropout=True`` adds the reference's
four dropout sites to that training forward and backward, with masks from the library's Philox stream: DESIGN.md section 20.
``train_lengths=True`` lets that forward take ``x_lengths`` / ``sem_lengths`` (ragged training batches): DESIGN.md section 22.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import native
from ._cache import PackedBlob, WorkspaceCache
from .synth import decoder_shapes, sinusoidal_table, time_frequencies


class _Node(nn.Module):
    """Parameter container; the tree of _Node objects reproduces the reference's dotted key names."""


def _attach(root: nn.Module, key: str, tensor: torch.Tensor, is_buffer: bool) -> None:
    *path, leaf = key.split(".")
    mod = root
    for name in path:
        if name not in mod._modules:
            mod.add_module(name, _Node())
        mod = mod._modules[name]
    if is_buffer:
        mod.register_buffer(leaf, tensor)
    else:
        mod.register_parameter(leaf, nn.Parameter(tensor, requires_grad=False))


# the decoder blob's byte-count query and pack call, looked up in native at call time (tests count packs by wrapping native.pack_weights)
def _packed_bytes(dims):
    return native.packed_bytes(dims)


def _pack_weights(dims, tensors, blob):
    native.pack_weights(dims, tensors, blob)


class _DecoderGrad(torch.autograd.Function):
    """eps = decoder(...) on the training forward (edtts_decoder_forward_train); backward through edtts_decoder_backward.  The tape is
    a tensor of this call's own, saved in ctx: any number of forwards may share the decoder's cached workspace before a backward.
    ``drop``: None, or the (p, seed) pair of this call's dropout masks; it lives in ctx, so the backward regenerates the masks of
    ITS forward whatever the decoder has run since.  ``lens``: (t_len, s_len), device int64 [B] or None each (train_lengths=True),
    kept in ctx for the backward as well."""

    @staticmethod
    def forward(ctx, dec, t, sem_idx, step_idx, names, drop, x_t, sem_features, lens, *params):
        B, T, _ = x_t.shape
        S = sem_features.shape[1] if sem_features is not None else sem_idx.shape[1]
        dims = dec.dims()
        packed = dec._ensure_packed(trainable=True)
        ws = dec.workspace(B, T, S, B, x_t.device)
        x = x_t.detach().contiguous()
        t = t.contiguous()
        step_idx = None if step_idx is None else step_idx.contiguous()
        sem_idx = None if sem_features is not None or sem_idx is None else sem_idx.contiguous()
        feats = None if sem_features is None else sem_features.detach().contiguous()
        tape = torch.empty(native.train_tape_bytes(dims, B, T, S), dtype=torch.uint8, device=x.device)
        eps = native.decoder_forward_train(dims, packed, ws, tape, x, t, step_idx, sem_idx, feats, S, drop, *lens)
        ctx.dec, ctx.names, ctx.S, ctx.sig, ctx.drop, ctx.lens = dec, names, S, dec._blob.sig, drop, lens
        ctx.inputs = (x, t, step_idx, sem_idx, feats)
        ctx.save_for_backward(tape, *params)
        return eps

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_eps):
        dec = ctx.dec
        tape, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        x, t, step_idx, sem_idx, feats = ctx.inputs
        if dec._blob.sig != ctx.sig:
            raise RuntimeError("EdgeDiffusionDecoder: a parameter was modified between this forward and its backward")
        B, T, _ = x.shape
        dims, packed = dec.dims(), dec._packed
        ws = dec.workspace(B, T, ctx.S, B, x.device)
        wanted = {n: p for n, p, need in zip(ctx.names, params, ctx.needs_input_grad[9:]) if need and dec._enters_output(n, feats is not None, step_idx is not None)}
        out = {n: torch.empty_like(p) for n, p in wanted.items()}
        slots = [out.get(dec._slot_param(n)) for n in native.slot_names(dec.cfg.layers)]
        d_x = torch.empty_like(x) if ctx.needs_input_grad[6] else None
        d_f = torch.empty_like(feats) if feats is not None and ctx.needs_input_grad[7] else None
        native.decoder_backward(dims, packed, ws, tape, x, t, step_idx, sem_idx, feats, ctx.S, d_eps.contiguous(), slots, d_x, d_f, ctx.drop,
                                *ctx.lens)
        return (None, None, None, None, None, None, d_x, d_f, None, *[out.get(n) for n in ctx.names])


class EdgeDiffusionDecoder(nn.Module):
    def __init__(self, cfg, max_len: int = 1000, max_context_len: int = 512, compute_dtype: str = "f32", kernels: str = "compiled",
                 autograd: bool = False, train_dropout: bool = False, train_lengths: bool = False, matmul_dtype: str = "f32",
                 attn_dtype: str = "f32", tape_dtype: str = "f32"):
        """``max_len`` / ``max_context_len`` size the two sinusoidal tables (reference: 1000 / 512, decoder.py:38,41);
        they are pure functions of position, so larger values only lift the reference's length limit.
        ``compute_dtype``: "f32" (the reference's arithmetic) or "bf16" -- contractions on bf16 MFMA with fp32 accumulation,
        residual stream / norms / softmax in fp32 (the reference's AMP precedent, utils/speed_utils.py:70; compiled for
        head_dim 32, i.e. BASELINE config 3: hidden=256, heads=8).  Parameters stay fp32 either way.
        ``kernels``: "compiled" (default) runs only shapes that are compiled kernel instances; "generic" runs every shape on the
        run-time-shape fp32 kernels; "auto" takes the compiled instance when there is one and the generic kernels otherwise
        (include/edtts.h: EDTTS_KERNELS_*).  The generic kernels are fp32 only.
        ``autograd``: False (default) -- ``forward`` is inference only, as before.  True (needs ``kernels="generic"`` and fp32) --
        the parameters require grad, and a ``forward`` under grad mode whose parameters, ``x_t`` or ``sem_features`` require grad is
        differentiable: it runs the training forward and hands ``backward()`` to the backward kernels.
        ``train_dropout``: False (default) -- a differentiable forward in training mode with ``cfg.dropout > 0`` raises, as before.
        True (needs ``autograd=True``) -- that forward applies the reference's dropout (attention probabilities of both attentions,
        after SwiGLU, after the FFN's down projection) with ``p = cfg.dropout``; each such forward draws a 63-bit seed on the host
        from ``self.dropout_generator`` (a CPU ``torch.Generator``; None, the default: torch's default CPU generator, so
        ``torch.manual_seed`` makes a run repeatable), keeps it for its own backward and shows it as ``self.last_dropout_seed``.
        With ``self.dropout_keys = (key_stream, first_slot)`` (a ``KeyStream``) each such forward instead takes a slot of the
        stream -- ``first_slot`` for this module's first forward since the stream's last ``advance()``, the next one for its second,
        and so on -- a key in device memory that the kernels read when they run, so a captured step draws new masks on every
        replay; ``last_dropout_seed`` is then None.
        The masks are the library's (include/edtts.h, "Dropout masks"), not torch's random stream.  ``.eval()``, ``cfg.dropout ==
        0`` and calls that are not differentiable are unchanged; in particular a training-mode call under ``torch.no_grad()`` runs
        the inference forward WITHOUT dropout (the reference would drop there too): DESIGN.md section 20.
        ``train_lengths``: False (default) -- a differentiable forward given ``x_lengths`` / ``sem_lengths`` raises, as before.  True
        (needs ``autograd=True``) -- that forward takes them (a ragged training batch): eps is bitwise the inference forward's with
        the same lengths (0 past ``x_lengths[b]``), the backward reads nothing past the lengths, padding contributes exactly nothing
        to any gradient, and ``x_t.grad`` / ``sem_features.grad`` are 0 there.  Composes with ``train_dropout``: DESIGN.md section 22.
        ``matmul_dtype``: "f32" (default) or "bf16" (needs ``kernels="generic"``) -- mixed precision on the generic kernels: every
        contraction the reference writes as a Linear, in the forward, the samplers' eps, the backward's dX and dW and its
        recomputed SwiGLU pre-activations, rounds both operands to bf16 and runs on bf16 MFMAs with fp32 accumulators.  Storage
        (which is what ``compute_dtype`` names) stays fp32: parameters, blob, tape, residual stream, norms, biases, softmax and both
        attentions, every output and gradient.  It rounds strictly less than ``torch.autocast`` does, so no GradScaler is needed.
        Composes with ``autograd``, ``train_dropout`` and ``train_lengths``: DESIGN.md section 26.
        ``attn_dtype``: "f32" (default) or "bf16" (needs ``kernels="generic"``) -- the other half of mixed precision, independent of
        ``matmul_dtype``: both attentions of every block, forward and backward, run their contractions (q k^T, p v, dO v^T, and the
        products that make dQ, dK and dV) on bf16 MFMAs with fp32 accumulators, as ``torch.autocast`` runs them.  Only the operands
        of those products are rounded; the scale, mask, softmax statistics, log-sum-exp, delta and every stored tensor stay fp32, and
        the dropout masks are the same.  Composes with everything ``matmul_dtype`` composes with: DESIGN.md section 27.
        ``tape_dtype``: "f32" (default) or "bf16" (needs ``kernels="generic"``, ``matmul_dtype="bf16"`` AND ``attn_dtype="bf16"``) --
        the four per-layer activations that, with both of those on, are read only by loaders that round to bf16 (q|k|v, the
        cross-attention queries, the cross K|V rows and the SwiGLU output) are stored as bf16, on the training tape and in the
        inference workspace alike.  Rounding to bf16 is idempotent, so eps, every gradient and every sampler output are BITWISE those
        of ``tape_dtype="f32"``; what changes is the tape (11 H -> 8 H floats per frame and layer at ffn_mult 2) and the traffic of
        those buffers.  Everything else stays fp32.  Composes with everything the other two compose with: DESIGN.md section 28."""
        super().__init__()
        if tape_dtype not in native.TAPE_DTYPES:
            raise ValueError(f"tape_dtype must be one of {sorted(native.TAPE_DTYPES)}, got {tape_dtype!r}")
        if native.TAPE_DTYPES[tape_dtype]:
            missing = ([f"kernels='generic' (got kernels={kernels!r})"] if kernels != "generic" else []) + [
                f"{k}='bf16' (got {k}={v!r})" for k, v, table in (("matmul_dtype", matmul_dtype, native.MATMUL_DTYPES),
                                                                  ("attn_dtype", attn_dtype, native.ATTN_DTYPES))
                if not table.get(v)]
            if missing:
                raise ValueError(f"tape_dtype={tape_dtype!r} needs " + " and ".join(missing) + ": a buffer with an fp32 reader cannot be "
                                 "stored as bf16 without changing results")
        self.tape_dtype = tape_dtype
        if attn_dtype not in native.ATTN_DTYPES:
            raise ValueError(f"attn_dtype must be one of {sorted(native.ATTN_DTYPES)}, got {attn_dtype!r}")
        if native.ATTN_DTYPES[attn_dtype] and kernels != "generic":
            raise ValueError(f"attn_dtype={attn_dtype!r} needs kernels='generic' (the bf16 attention kernels are built for the generic "
                             f"kernels only), got kernels={kernels!r}")
        self.attn_dtype = attn_dtype
        if matmul_dtype not in native.MATMUL_DTYPES:
            raise ValueError(f"matmul_dtype must be one of {sorted(native.MATMUL_DTYPES)}, got {matmul_dtype!r}")
        if native.MATMUL_DTYPES[matmul_dtype] and kernels != "generic":
            raise ValueError(f"matmul_dtype={matmul_dtype!r} needs kernels='generic' (the bf16 products are built for the generic "
                             f"kernels only), got kernels={kernels!r}")
        self.matmul_dtype = matmul_dtype
        self.autograd = bool(autograd)
        self.train_dropout = bool(train_dropout)
        self.train_lengths = bool(train_lengths)
        if self.train_lengths and not self.autograd:
            raise ValueError("train_lengths=True needs autograd=True (the lengths belong to the training forward and its backward)")
        if self.train_dropout and not self.autograd:
            raise ValueError("train_dropout=True needs autograd=True (dropout belongs to the training forward and its backward)")
        self.dropout_generator: Optional[torch.Generator] = None
        self.last_dropout_seed: Optional[int] = None
        self.dropout_keys = None  # (KeyStream, first slot): dropout keys from device memory instead of host draws
        if self.autograd and kernels != "generic":
            raise ValueError(f"autograd=True needs kernels='generic' (the backward differentiates the generic kernels), got {kernels!r}")
        if self.autograd and native.COMPUTE_DTYPES.get(compute_dtype) != native.COMPUTE_DTYPES["f32"]:
            raise ValueError(f"autograd=True needs compute_dtype='f32' (the backward is fp32 only), got {compute_dtype!r}")
        self.cfg = cfg
        if compute_dtype not in native.COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(native.COMPUTE_DTYPES)}, got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        if kernels not in native.KERNELS:
            raise ValueError(f"kernels must be one of {sorted(native.KERNELS)}, got {kernels!r}")
        if kernels != "compiled" and native.COMPUTE_DTYPES[compute_dtype] != native.COMPUTE_DTYPES["f32"]:
            raise ValueError(f"kernels={kernels!r} needs compute_dtype='f32' (the generic kernels are fp32 only), got {compute_dtype!r}")
        self.kernels = kernels
        self.max_len, self.max_context_len, self.n_step_emb = int(max_len), int(max_context_len), 16
        H = cfg.hidden
        for key, shape in decoder_shapes(cfg, self.max_len, self.max_context_len, self.n_step_emb).items():
            if key == "pos_emb.pe":
                _attach(self, key, sinusoidal_table(self.max_len, H), True)
            elif key == "context_pos_emb.pe":
                _attach(self, key, sinusoidal_table(self.max_context_len, H), True)
            else:
                _attach(self, key, self._default_init(key, shape), False)
        self._fix_bias_init()
        if self.autograd:
            for p in self.parameters():
                p.requires_grad_(True)
        self.register_buffer("_time_freqs", time_frequencies(H), persistent=False)
        self._zero_mod = None
        self._blob = PackedBlob(_packed_bytes, _pack_weights)  # (_cache.py: copies get bookkeeping of their own)
        self._ws = WorkspaceCache()

    # same distributions as the reference's default construction (nn.Linear / nn.Embedding defaults, ones for norm
    # gains, zeros for final out_proj and the AdaLN projections -- decoder.py:63-64, transformer.py:61-62)
    @staticmethod
    def _default_init(key: str, shape) -> torch.Tensor:
        leaf = key.rsplit(".", 1)[-1]
        if key.startswith("out_proj.") or ".norm1.proj." in key or ".norm3.proj." in key:
            return torch.zeros(shape)
        if key.endswith("emb.weight"):
            return torch.randn(shape)
        if "norm" in key and leaf == "weight" and len(shape) == 1:
            return torch.ones(shape)
        if key == "final_norm.bias":
            return torch.zeros(shape)
        if leaf == "weight":
            bound = 1.0 / math.sqrt(shape[-1])
            return torch.empty(shape).uniform_(-bound, bound)
        return torch.zeros(shape)  # Linear biases: drawn in _fix_bias_init (needs the sibling weight's fan-in)

    def _fix_bias_init(self) -> None:
        sd = dict(self.named_parameters())
        for k, p in sd.items():
            if k.endswith(".bias") and not (k.startswith("out_proj.") or ".norm1.proj." in k or ".norm3.proj." in k or k == "final_norm.bias"):
                w = sd[k[:-4] + "weight"]
                bound = 1.0 / math.sqrt(w.shape[-1])
                with torch.no_grad():
                    p.uniform_(-bound, bound)

    def reset_parameters(self) -> None:
        self._fix_bias_init()

    # ------------------------------------------------------------------------------------------ checkpoint interop
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts the reference's decoder state-dicts as they are saved in practice: plain keys
        (train.py:195,291-297; generate_sample.py:51) and keys prefixed with ``_orig_mod.`` when the decoder had been
        wrapped by torch.compile before saving (train.py:84-86 + :195; only train_v2.py:339 unwraps it).  Tensors are
        converted to fp32; positional tables shorter/longer than this module's are rejected by the normal shape check."""
        sd = {}
        for k, v in state_dict.items():
            k = k[len("_orig_mod."):] if k.startswith("_orig_mod.") else k
            if k.endswith("rope.cos_cached") or k.endswith("rope.sin_cached"):  # non-persistent in the reference, tolerated
                continue
            sd[k] = v.to(torch.float32) if torch.is_tensor(v) and v.is_floating_point() else v
        return super().load_state_dict(sd, strict=strict, **kw)

    @classmethod
    def from_checkpoint(cls, checkpoint, cfg=None, device=None, **kw) -> "EdgeDiffusionDecoder":
        """Build a decoder from a reference checkpoint dict (or a path to one): ``{"decoder": state_dict, "cfg": dict, ...}``
        as written by train.py:291-297 / train_v2.py:335-341 and read by generate_sample.py:38-51.  ``cfg`` overrides the
        stored config; ``codebook_size`` follows the checkpoint's token embedding (FSQ runs have 2304 codes, train_v2.py:246)."""
        from .config import CFG
        if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, "__fspath__"):
            checkpoint = torch.load(checkpoint, map_location="cpu", weights_only=False)
        sd = checkpoint["decoder"] if "decoder" in checkpoint else checkpoint
        if cfg is None:
            stored = checkpoint.get("cfg") if isinstance(checkpoint, dict) else None
            if stored is None:
                cfg = CFG()
            elif isinstance(stored, dict):
                cfg = CFG.from_dict(dict(stored))
            else:  # a pickled reference CFG object: copy the fields both classes share
                cfg = CFG.from_dict({k: getattr(stored, k) for k in CFG.__dataclass_fields__ if hasattr(stored, k) and k != "phase"})
        tok = next((v for k, v in sd.items() if k.endswith("token_emb.weight")), None)
        if tok is not None and tok.shape[0] != cfg.codebook_size:
            cfg.codebook_size = int(tok.shape[0])
        pe = next((v for k, v in sd.items() if k.endswith("pos_emb.pe") and "context" not in k), None)
        cpe = next((v for k, v in sd.items() if k.endswith("context_pos_emb.pe")), None)
        dec = cls(cfg, max_len=int(pe.shape[0]) if pe is not None else 1000,
                  max_context_len=int(cpe.shape[0]) if cpe is not None else 512, **kw)
        dec.load_state_dict(sd)
        if device is not None:
            dec = dec.to(device)
        return dec.eval()

    # ------------------------------------------------------------------------------------------ native state
    def dims(self) -> native.EdttsDims:
        c = self.cfg
        window = -1 if c.attn_window_size is None else int(c.attn_window_size)
        return native.EdttsDims(c.hidden, c.layers, c.heads, c.n_mels, c.ffn_mult, c.codebook_size, c.semantic_dim, window,
                                self.max_len, self.max_context_len, self.n_step_emb,
                                native.COMPUTE_DTYPES[self.compute_dtype] | native.KERNELS[self.kernels]
                                | native.MATMUL_DTYPES[self.matmul_dtype] | native.ATTN_DTYPES[self.attn_dtype]
                                | native.TAPE_DTYPES[self.tape_dtype])

    def _state_tensors(self) -> Dict[str, torch.Tensor]:
        sd = {k: v for k, v in self.named_parameters()}
        sd.update({k: v for k, v in self.named_buffers()})
        sd["time_freqs"] = sd.pop("_time_freqs")
        if not self.cfg.use_adaln:
            # Plain RMSNorm blocks (layers/transformer.py:101-104,119-122,142-157): the kernels' AdaLN slots get the RMSNorm
            # gain and an all-zero modulation projection, i.e. (1 + scale, shift) = (1, 0) -- y * 1 + 0 is exact in fp32.
            H = self.cfg.hidden
            dev = sd["in_proj.weight"].device
            if self._zero_mod is None or self._zero_mod[0].device != dev:
                self._zero_mod = (torch.zeros(2 * H, H, device=dev), torch.zeros(2 * H, device=dev))
            for l in range(self.cfg.layers):
                for n in ("norm1", "norm3"):
                    sd[f"layers.{l}.{n}.norm.weight"] = sd.pop(f"layers.{l}.{n}.weight")
                    sd[f"layers.{l}.{n}.proj.weight"], sd[f"layers.{l}.{n}.proj.bias"] = self._zero_mod
        return sd

    def _slot_tensors(self):
        """(slot names, tensors in slot order).  Building the name -> tensor map through named_parameters() walks the module tree and
        formats ~90 dotted names (245 us per call on the build container's host, a third of a B = 1 sampler call).  The tree of
        containers is fixed after construction, so each slot is resolved ONCE to (the owning module's _parameters / _buffers dict,
        key) and read from there on every call: a parameter that was written into, moved by .to() or replaced by a new Parameter
        object is picked up all the same (12 us)."""
        if not self.cfg.use_adaln:  # (plain-RMSNorm decoders substitute tensors for the AdaLN slots: the general path)
            sd = self._state_tensors()
            names = native.slot_names(self.cfg.layers)
            return names, [sd[n] for n in names]
        refs = getattr(self, "_slot_refs", None)
        if refs is None:
            names = native.slot_names(self.cfg.layers)
            pairs = []
            for n in names:
                key = "_time_freqs" if n == "time_freqs" else n
                *path, leaf = key.split(".")
                mod = self
                for part in path:
                    mod = mod._modules[part]
                pairs.append((mod._parameters if leaf in mod._parameters else mod._buffers, leaf))
            refs = self._slot_refs = (names, pairs)
        return refs[0], [d[k] for d, k in refs[1]]

    def _ensure_packed(self, trainable: bool = False) -> torch.Tensor:
        """The packed weight blob, (re-)packed on the current stream when a parameter has changed; a call on another stream is
        ordered behind the pack (PackedBlob.get).  Changing parameters while calls that read the old blob are
        still in flight on other streams is the caller's to order, as for any module.  ``trainable``: PackedBlob.get's (the
        differentiable forward passes True: under graph capture an unmirrored blob is packed inside the capture)."""
        names, tensors = self._slot_tensors()
        return self._blob.get(self.dims(), tensors, names=names, trainable=trainable)

    _packed = property(lambda self: self._blob.blob)
    _workspaces = property(lambda self: self._ws.entries)
    _pinned_workspaces = property(lambda self: self._ws.pinned)

    # ------------------------------------------------------------------------------------------ blob mirror (optim.FusedAdamW)
    def _mirror_map(self) -> Optional[Dict[str, Tuple[int, int, int, bool]]]:
        """{parameter name: (offset in floats, rows, cols, transposed)} of the packed blob, from the library's own layout
        (native.generic_slot_dest); None for a decoder whose blob is not the generic fp32 one (fragment-order blobs are not mirrored)."""
        if self.kernels != "generic" or native.COMPUTE_DTYPES[self.compute_dtype] != native.COMPUTE_DTYPES["f32"]:
            return None
        dims, out = self.dims(), {}
        for i, slot in enumerate(native.slot_names(self.cfg.layers)):
            name = self._slot_param(slot)
            if name is not None:
                out[name] = native.generic_slot_dest(dims, i)
        return out

    def _mirror_target(self) -> Optional[torch.Tensor]:
        """The packed blob if it is current -- packed, and packed from the tensors as they stand -- else None.  The current stream is
        ordered behind the pack, so an optimiser step enqueued on it may write the new values into the blob."""
        return self._blob.current(self.dims(), self._slot_tensors()[1])

    def _mirror_commit(self) -> None:
        """After a step that wrote every updated parameter into the blob as well and bumped the parameters' versions: the blob is
        current again.  Takes the signature of the tensors as they stand and records the pack event on the current stream."""
        self._blob.commit(self.dims(), self._slot_tensors()[1])

    WORKSPACE_CACHE = 8

    def workspace(self, B: int, T: int, S: int, cond_rows: int, device, tag: str = "", *, stream=None) -> torch.Tensor:
        """Cached scratch memory for one (shape, device, tag, sub-batch cut, stream): WorkspaceCache's rules (one per stream, at most
        WORKSPACE_CACHE kept, pinned while a captured graph may replay into it).  A workspace is allocated and zero-filled on the
        stream it belongs to -- ``stream``, by default the device's current stream.  The key also holds the number of sub-batches a
        sampler call of this shape makes under the current edtts_set_substreams setting (native.substreams_for), so a setting change
        never hands out a workspace laid out for another cut."""
        dims = self.dims()

        def alloc():
            nbytes = native.workspace_bytes(dims, B, T, S, cond_rows)
            if stream is not None and torch.device(device).type == "cuda" and stream.cuda_stream != torch.cuda.current_stream(device).cuda_stream:
                with torch.cuda.stream(stream):
                    return torch.zeros(nbytes, dtype=torch.uint8, device=device)
            return torch.zeros(nbytes, dtype=torch.uint8, device=device)  # must start zero-filled (padding lanes)

        head = (B, T, S, cond_rows, str(device), tag, native.substreams_for(dims, B, T))  # (the cut: a host query)
        return self._ws.get(self, head, device, stream, alloc)

    def release_pinned(self, B: Optional[int] = None, T: Optional[int] = None, S: Optional[int] = None) -> int:
        """Un-pin (and drop) the workspaces that were handed out during graph capture -- all of them, or those of one (B, T, S): call
        this once the graphs that replay into them have been destroyed (WorkspaceCache.release_pinned).  Returns their number."""
        return self._ws.release_pinned(lambda k: (B is None or k[0] == B) and (T is None or k[1] == T) and (S is None or k[2] == S))

    # ------------------------------------------------------------------------------------------ autograd
    def _slot_param(self, slot: str) -> Optional[str]:
        """The parameter a weight slot's gradient belongs to (None: a buffer, or a slot this decoder fills with a constant)."""
        if slot in ("pos_emb.pe", "context_pos_emb.pe", "time_freqs"):
            return None
        if not self.cfg.use_adaln:  # plain RMSNorm blocks: the gain sits in the AdaLN slot, the modulation slots hold zeros
            if ".norm1.proj." in slot or ".norm3.proj." in slot:
                return None
            return slot.replace(".norm1.norm.weight", ".norm1.weight").replace(".norm3.norm.weight", ".norm3.weight")
        return slot

    def _enters_output(self, name: str, with_features: bool, with_step: bool) -> bool:
        """False for the parameters torch itself would leave without a gradient for this call."""
        if name == "token_emb.weight":
            return not with_features
        if name.startswith("sem_proj."):
            return with_features
        if name.startswith("time_emb."):
            return bool(self.cfg.use_adaln)
        if name == "step_emb.weight":
            return with_step and bool(self.cfg.use_adaln)
        return True

    def _named_params(self):
        """(names, parameters) without walking the module tree on every call: the tree of containers is fixed after construction,
        so each parameter is resolved once to (its owner's _parameters dict, key) and read from there (see _slot_tensors)."""
        refs = getattr(self, "_param_refs", None)
        if refs is None:
            names, pairs = [], []
            for prefix, mod in self.named_modules():
                for leaf in mod._parameters:
                    names.append(f"{prefix}.{leaf}" if prefix else leaf)
                    pairs.append((mod._parameters, leaf))
            refs = self._param_refs = (tuple(names), pairs)
        return refs[0], tuple(d[k] for d, k in refs[1])

    def _forward_autograd(self, x_t, t, sem_idx, step_idx, sem_features, x_lengths, sem_lengths) -> torch.Tensor:
        if sem_idx is None and sem_features is None:
            raise ValueError("Either sem_idx or sem_features must be provided")
        lens = (None, None)
        if x_lengths is not None or sem_lengths is not None:
            if not self.train_lengths:
                raise ValueError("autograd=True: x_lengths / sem_lengths are not supported by the backward (pad-free batches only) "
                                 "unless the decoder was built with train_lengths=True")
            B, T, _ = x_t.shape
            S = sem_features.shape[1] if sem_features is not None else sem_idx.shape[1]
            lens = (native.lengths(x_lengths, B, T, x_t.device, "x_lengths"), native.lengths(sem_lengths, B, S, x_t.device, "sem_lengths"))
        drop = None
        if self.training and self.cfg.dropout > 0 and self.train_dropout and self.dropout_keys is not None:
            drop = native.DropKey(float(self.cfg.dropout), self.dropout_keys[0].take(self, self.dropout_keys[1]))  # (kept in ctx for this forward's backward)
            self.last_dropout_seed = None
        elif self.training and self.cfg.dropout > 0 and self.train_dropout:
            # (a host draw from a CPU generator: no device work, no synchronisation)
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=self.dropout_generator).item())
            drop = (float(self.cfg.dropout), seed)
            self.last_dropout_seed = seed
        elif self.training and self.cfg.dropout > 0:
            raise ValueError(f"autograd=True: the kernels have no dropout but cfg.dropout={self.cfg.dropout} and the decoder is in "
                             "training mode (the reference applies attention and FFN dropout there): set cfg.dropout = 0 or call .eval()")
        names, params = self._named_params()
        return _DecoderGrad.apply(self, t, sem_idx, step_idx, names, drop, x_t, sem_features, lens, *params)

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, x_t: torch.Tensor, t: torch.Tensor, sem_idx: Optional[torch.Tensor] = None,
                step_idx: Optional[torch.Tensor] = None, sem_features: Optional[torch.Tensor] = None, *,
                x_lengths: Optional[torch.Tensor] = None, sem_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """See ``_forward_inference`` for the arguments.  With ``autograd=True``, under grad mode and with something that requires
        grad (a parameter, ``x_t`` or ``sem_features``), the result is differentiable; otherwise this is the inference forward."""
        if self.autograd and torch.is_grad_enabled() and (
                x_t.requires_grad or (sem_features is not None and sem_features.requires_grad)
                or any(p.requires_grad for p in self._named_params()[1])):
            return self._forward_autograd(x_t, t, sem_idx, step_idx, sem_features, x_lengths, sem_lengths)
        return self._forward_inference(x_t, t, sem_idx, step_idx, sem_features, x_lengths=x_lengths, sem_lengths=sem_lengths)

    @torch.no_grad()
    def _forward_inference(self, x_t: torch.Tensor, t: torch.Tensor, sem_idx: Optional[torch.Tensor] = None,
                step_idx: Optional[torch.Tensor] = None, sem_features: Optional[torch.Tensor] = None, *,
                x_lengths: Optional[torch.Tensor] = None, sem_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eps = decoder(x_t [B,T,n_mels], t [B], sem_idx [B,S] | sem_features [B,S,semantic_dim], step_idx [B] | None).

        ``x_lengths`` / ``sem_lengths`` (int64 [B], optional): utterance b has that many valid frames / tokens (a ragged batch,
        DESIGN.md section 11).  Row b on its frames is then bitwise what the call on utterance b alone returns, nothing past the
        lengths is read, and eps is 0 past x_lengths[b].  See native.lengths for CPU versus device length tensors."""
        if sem_idx is None and sem_features is None:
            raise ValueError("Either sem_idx or sem_features must be provided")
        B, T, _ = x_t.shape
        S = sem_features.shape[1] if sem_features is not None else sem_idx.shape[1]
        t_len = native.lengths(x_lengths, B, T, x_t.device, "x_lengths")
        s_len = native.lengths(sem_lengths, B, S, x_t.device, "sem_lengths")
        packed = self._ensure_packed()
        ws = self.workspace(B, T, S, B, x_t.device)
        return native.decoder_forward(self.dims(), packed, ws, x_t.contiguous(), t.contiguous(),
                                      None if step_idx is None else step_idx.contiguous(),
                                      None if sem_features is not None or sem_idx is None else sem_idx.contiguous(),
                                      None if sem_features is None else sem_features.contiguous(), S, t_len, s_len)
