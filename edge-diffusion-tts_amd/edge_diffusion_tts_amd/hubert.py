"""NativeHubert -- transformers' HubertModel forward (hubert-base layout) on this package's gfx950 kernels.

``NativeHubert(config, num_layers)(wav)`` equals ``HubertModel(wav, output_hidden_states=True).hidden_states[num_layers]`` in eval mode,
fp32, and runs only the layers up to ``num_layers`` (the reference reads layer 9 of 12: models/encoder.py, inference_pipeline.py:40-43).
The whole forward is one C call (edtts_hubert_forward, csrc/edtts_hubert.h): no CPU path, no fall-back to the torch model.

State-dict keys are transformers' own.  The positional conv loads from either stored form of its weight norm
(``conv.parametrizations.weight.original0/1`` as transformers writes it now, or ``conv.weight_g/weight_v`` of older checkpoints
such as hubert-base-ls960); the weight norm is folded into the conv weight when the weights are packed.  ``masked_spec_embed`` and
the layers past ``num_layers`` are ignored.

``lengths`` (int64 [B] sample counts) makes row b equal to the call on ``wav[b:b+1, :lengths[b]]`` alone, bitwise: per-utterance
GroupNorm statistics, positional-conv padding and attention keys -- which transformers' padded batch cannot give (hubert-base's
GroupNorm normalises over the whole padded time axis).

``compute_dtype="bf16"`` (default ``"fp32"``) runs every contraction after conv0 -- the conv stack, the feature projection, the
positional conv, QKV, the attention products, out_proj, the FFN -- on bf16 MFMAs with fp32 accumulators (csrc/edtts_hubert16.h);
conv0, the GroupNorm, the residual stream, every LayerNorm, GELU, the softmax and the output stay fp32.  The parameters stay fp32
``nn.Parameter``s under transformers' keys: only the packed blob and the workspace differ.  Every invariance above holds bitwise.
"""
from __future__ import annotations

from functools import partial
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import native
from ._cache import PackedBlob, WorkspaceCache

# transformers.HubertConfig defaults (hubert-base) for fields a dict may leave out
_DEFAULTS = dict(
    hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu", layer_norm_eps=1e-5,
    feat_extract_norm="group", feat_extract_activation="gelu", conv_dim=(512, 512, 512, 512, 512, 512, 512),
    conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_bias=False, num_conv_pos_embeddings=128,
    num_conv_pos_embedding_groups=16, do_stable_layer_norm=False, feat_proj_layer_norm=True, conv_pos_batch_norm=False)
_POS_G = "encoder.pos_conv_embed.conv.parametrizations.weight.original0"
_POS_V = "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
_POS_OLD = {"encoder.pos_conv_embed.conv.weight_g": _POS_G, "encoder.pos_conv_embed.conv.weight_v": _POS_V}
_LAYER_KEYS = ("attention.q_proj.weight", "attention.q_proj.bias", "attention.k_proj.weight", "attention.k_proj.bias",
               "attention.v_proj.weight", "attention.v_proj.bias", "attention.out_proj.weight", "attention.out_proj.bias",
               "layer_norm.weight", "layer_norm.bias", "feed_forward.intermediate_dense.weight", "feed_forward.intermediate_dense.bias",
               "feed_forward.output_dense.weight", "feed_forward.output_dense.bias", "final_layer_norm.weight", "final_layer_norm.bias")


def _cfg_get(config, name):
    if isinstance(config, dict):
        return config.get(name, _DEFAULTS[name])
    return getattr(config, name, _DEFAULTS[name])


def _act_name(v) -> str:
    return v if isinstance(v, str) else type(v).__name__


class NativeHubert(nn.Module):
    """hidden_states[num_layers] of transformers' HubertModel on the kernels (see the module docstring)."""

    WORKSPACE_CACHE = 8

    def __init__(self, config, num_layers: int, compute_dtype: str = "fp32"):
        super().__init__()
        if compute_dtype not in native.HUBERT_DTYPES:
            raise ValueError(f"NativeHubert: compute_dtype={compute_dtype!r}: expected one of {sorted(native.HUBERT_DTYPES)}")
        self.compute_dtype = compute_dtype
        self._dt = native.HUBERT_DTYPES[compute_dtype]
        c = {k: _cfg_get(config, k) for k in _DEFAULTS}
        self.config_dict = c
        need = (("feat_extract_norm", "group"), ("do_stable_layer_norm", False), ("conv_bias", False), ("feat_proj_layer_norm", True),
                ("conv_pos_batch_norm", False))
        for name, want in need:
            if c[name] != want:
                raise native.EdttsError(f"NativeHubert: {name}={c[name]!r} is not supported (the hubert-base layout needs {want!r})")
        for name in ("feat_extract_activation", "hidden_act"):
            if _act_name(c[name]) != "gelu":
                raise native.EdttsError(f"NativeHubert: {name}={c[name]!r} is not supported (the kernels implement the erf GELU, 'gelu')")
        H, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
        if heads < 1 or H % heads:
            raise native.EdttsError(f"NativeHubert: hidden_size={H} is not a multiple of num_attention_heads={heads}")
        if H // heads > 128:
            raise native.EdttsError(f"NativeHubert: head_dim = hidden_size / num_attention_heads = {H // heads} > 128")
        n_conv = len(c["conv_dim"])
        if not (len(c["conv_kernel"]) == len(c["conv_stride"]) == n_conv) or not 1 <= n_conv <= 16:
            raise native.EdttsError(f"NativeHubert: conv_dim, conv_kernel and conv_stride need the same length in 1..16, got "
                                    f"{len(c['conv_dim'])}, {len(c['conv_kernel'])}, {len(c['conv_stride'])}")
        n_total = int(c["num_hidden_layers"])
        if not 0 <= int(num_layers) <= n_total:
            raise ValueError(f"NativeHubert: num_layers={num_layers} outside [0, num_hidden_layers={n_total}]")
        self.num_layers = int(num_layers)
        self.hidden_size = H
        self.conv_kernel = [int(v) for v in c["conv_kernel"]]
        self.conv_stride = [int(v) for v in c["conv_stride"]]
        d = native.EdttsHubertDims()
        d.n_conv = n_conv
        for i in range(n_conv):
            d.conv_dim[i], d.conv_kernel[i], d.conv_stride[i] = int(c["conv_dim"][i]), self.conv_kernel[i], self.conv_stride[i]
        d.hidden, d.heads, d.intermediate, d.num_layers = H, heads, int(c["intermediate_size"]), self.num_layers
        d.pos_kernel, d.pos_groups = int(c["num_conv_pos_embeddings"]), int(c["num_conv_pos_embedding_groups"])
        d.layer_norm_eps = float(c["layer_norm_eps"])
        self.dims = d
        if self._dt:  # the limits only this dtype has (EdttsError naming the field); fp32 meets the library's at the first call, as before
            native.hubert_packed_bytes(d, self._dt)
        for key, shape in self._shapes():
            self._put(key, shape)
        self._register_load_state_dict_pre_hook(self._normalise_keys)
        self._blob = PackedBlob(partial(native.hubert_packed_bytes, compute_dtype=self._dt),
                                partial(native.hubert_pack, compute_dtype=self._dt), "NativeHubert weight")
        self._ws = WorkspaceCache()

    # ------------------------------------------------------------------------------------------ parameters
    def _shapes(self) -> List[Tuple[str, tuple]]:
        c, d = self.config_dict, self.dims
        C = [int(v) for v in c["conv_dim"]]
        H, I, pk, G = d.hidden, d.intermediate, d.pos_kernel, d.pos_groups
        fe = "feature_extractor.conv_layers."
        out = [(fe + "0.conv.weight", (C[0], 1, self.conv_kernel[0])), (fe + "0.layer_norm.weight", (C[0],)),
               (fe + "0.layer_norm.bias", (C[0],))]
        out += [(f"{fe}{i}.conv.weight", (C[i], C[i - 1], self.conv_kernel[i])) for i in range(1, len(C))]
        out += [("feature_projection.layer_norm.weight", (C[-1],)), ("feature_projection.layer_norm.bias", (C[-1],)),
                ("feature_projection.projection.weight", (H, C[-1])), ("feature_projection.projection.bias", (H,)),
                (_POS_G, (1, 1, pk)), (_POS_V, (H, H // G, pk)), ("encoder.pos_conv_embed.conv.bias", (H,)),
                ("encoder.layer_norm.weight", (H,)), ("encoder.layer_norm.bias", (H,))]
        shp = {"q": (H, H), "k": (H, H), "v": (H, H), "o": (H, H)}
        for l in range(self.num_layers):
            for k in _LAYER_KEYS:
                if k.endswith("norm.weight") or k.endswith("norm.bias"):
                    s = (H,)
                elif "intermediate_dense" in k:
                    s = (I, H) if k.endswith("weight") else (I,)
                elif "output_dense" in k:
                    s = (H, I) if k.endswith("weight") else (H,)
                else:
                    s = shp[k.split(".")[1][0]] if k.endswith("weight") else (H,)
                out.append((f"encoder.layers.{l}.{k}", s))
        return out

    def _put(self, key: str, shape) -> None:
        *path, name = key.split(".")
        m = self
        for p in path:
            if p not in m._modules:
                m.add_module(p, nn.Module())
            m = m._modules[p]
        init = torch.ones(shape) if name == "weight" and len(shape) == 1 else torch.zeros(shape)
        m.register_parameter(name, nn.Parameter(init, requires_grad=False))

    def _get(self, key: str) -> torch.Tensor:
        m = self
        *path, name = key.split(".")
        for p in path:
            m = m._modules[p]
        return getattr(m, name)

    def _normalise_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Before loading: the old weight-norm keys become the parametrization keys; masked_spec_embed and the layers past
        num_layers are dropped (they are not run)."""
        for old, new in _POS_OLD.items():
            if prefix + old in state_dict:
                state_dict[prefix + new] = state_dict.pop(prefix + old)
        state_dict.pop(prefix + "masked_spec_embed", None)
        lp = prefix + "encoder.layers."
        for k in [k for k in state_dict if k.startswith(lp)]:
            idx = k[len(lp):].split(".", 1)[0]
            if idx.isdigit() and int(idx) >= self.num_layers:
                del state_dict[k]

    def folded_pos_conv_weight(self) -> torch.Tensor:
        """The positional conv's weight with its weight norm (dim=2) folded in: w[:, :, k] = g[k] v[:, :, k] / |v[:, :, k]|."""
        return torch._weight_norm(self._get(_POS_V), self._get(_POS_G), 2)

    def _slots(self) -> List[torch.Tensor]:
        c = self.config_dict
        fe = "feature_extractor.conv_layers."
        keys = [fe + "0.conv.weight", fe + "0.layer_norm.weight", fe + "0.layer_norm.bias"]
        keys += [f"{fe}{i}.conv.weight" for i in range(1, len(c["conv_dim"]))]
        keys += ["feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias", "feature_projection.projection.weight",
                 "feature_projection.projection.bias"]
        t = [self._get(k) for k in keys] + [self.folded_pos_conv_weight()]
        t += [self._get(k) for k in ("encoder.pos_conv_embed.conv.bias", "encoder.layer_norm.weight", "encoder.layer_norm.bias")]
        for l in range(self.num_layers):
            t += [self._get(f"encoder.layers.{l}.{k}") for k in _LAYER_KEYS]
        return t

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_hubert(cls, model: nn.Module, num_layers: int, compute_dtype: str = "fp32") -> "NativeHubert":
        """From a transformers HubertModel (its config and state_dict); on the model's device."""
        m = cls(model.config, num_layers, compute_dtype=compute_dtype)
        m.load_state_dict(model.state_dict())
        dev = next(model.parameters()).device
        return m.to(dev).eval()

    @classmethod
    def from_pretrained(cls, hubert_id: str, num_layers: int, local_files_only: bool = True,
                        compute_dtype: str = "fp32") -> "NativeHubert":
        """Load ``hubert_id`` from the local Hugging Face cache only (never the network); raises SemanticEncoder's error when the
        model is not there."""
        from .encoder import _missing_hubert
        try:
            from transformers import HubertModel
        except ImportError as e:
            raise _missing_hubert(hubert_id, e) from e
        try:
            model = HubertModel.from_pretrained(hubert_id, local_files_only=True)
        except OSError as e:
            raise _missing_hubert(hubert_id, e) from e
        return cls.from_hubert(model, num_layers, compute_dtype=compute_dtype)

    # ------------------------------------------------------------------------------------------ lengths
    def frames(self, n_samples: int) -> int:
        """Output frames of n_samples of audio (transformers' _get_feat_extract_output_lengths); 0 when there is none."""
        n = int(n_samples)
        for k, s in zip(self.conv_kernel, self.conv_stride):
            n = (n - k) // s + 1
        return max(n, 0)

    def min_samples(self) -> int:
        """The shortest input that yields one frame (400 at the hubert-base defaults)."""
        r = 1
        for k, s in zip(reversed(self.conv_kernel), reversed(self.conv_stride)):
            r = (r - 1) * s + k
        return r

    def frames_of(self, lengths: torch.Tensor, T_audio: int) -> torch.Tensor:
        """Per-utterance frame counts of an int64 sample-count tensor, on its device (no host synchronisation), with the kernels'
        clamping of the sample counts into [min_samples(), T_audio]."""
        n = lengths.clamp(self.min_samples(), int(T_audio))
        for k, s in zip(self.conv_kernel, self.conv_stride):
            n = torch.div(n - k, s, rounding_mode="floor") + 1
        return n

    # ------------------------------------------------------------------------------------------ the forward
    def _packed(self) -> torch.Tensor:
        """The packed blob (PackedBlob.get).  The signature is taken over the parameters; what is packed is
        _slots(), which folds the weight norm into a fresh tensor, so it is built on a miss only."""
        return self._blob.get(self.dims, list(self.parameters()), packs=self._slots)

    _workspaces = property(lambda self: self._ws.entries)
    _pinned = property(lambda self: self._ws.pinned)

    def workspace(self, B: int, T_audio: int, device) -> torch.Tensor:
        """Cached scratch memory per (B, T_audio, device, stream), as EdgeDiffusionDecoder.workspace (WorkspaceCache, DESIGN.md section
        10): calls on several streams never share one; while a stream captures a graph it takes its own workspace or, failing that,
        the most recently used one of that shape (the eager warm-up's), which then stays pinned until release_pinned."""
        dev = torch.device(device)
        return self._ws.get(self, (B, T_audio, str(dev)), dev, None, lambda: torch.empty(
            native.hubert_workspace_bytes(self.dims, B, T_audio, self._dt), dtype=torch.uint8, device=dev))

    def release_pinned(self, B: Optional[int] = None, T_audio: Optional[int] = None) -> int:
        """Un-pin (and drop) the workspaces handed out during graph capture -- all, or those of one (B, T_audio) -- once their graphs
        have been destroyed (WorkspaceCache.release_pinned).  Returns their number."""
        return self._ws.release_pinned(lambda k: (B is None or k[0] == B) and (T_audio is None or k[1] == T_audio))

    @torch.no_grad()
    def forward(self, wav: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """wav fp32 [B, T_audio] on the GPU -> hidden_states[num_layers] [B, frames(T_audio), hidden].  lengths: optional int64 [B]
        sample counts; row b then equals the call on wav[b:b+1, :lengths[b]] alone and its rows past frames(lengths[b]) are 0."""
        if not isinstance(wav, torch.Tensor) or wav.dim() != 2:
            raise ValueError(f"NativeHubert: expected a waveform [B, T_audio], got {getattr(wav, 'shape', type(wav))}")
        if not wav.is_cuda:
            raise native.EdttsError(f"wav: expected a tensor on the HIP device, got {wav.device} -- NativeHubert has no CPU path")
        B, T_audio = wav.shape
        T = self.frames(T_audio)
        if T < 1:
            raise ValueError(f"NativeHubert: {T_audio} samples give no feature frame (need at least {self.min_samples()})")
        if B == 0:
            return torch.empty((0, T, self.hidden_size), dtype=torch.float32, device=wav.device)
        if lengths is not None and isinstance(lengths, torch.Tensor) and not lengths.is_cuda and lengths.numel() == B and B:
            if int(lengths.min()) < self.min_samples():
                raise ValueError(f"lengths: {int(lengths.min())} samples give no feature frame (need at least {self.min_samples()})")
        n = native.lengths(lengths, B, T_audio, wav.device, "lengths")
        wav = wav.float().contiguous()
        blob = self._packed()
        out = torch.empty((B, T, self.hidden_size), dtype=torch.float32, device=wav.device)
        native.hubert_forward(self.dims, blob, wav, n, out, self.workspace(B, T_audio, wav.device), self._dt)
        return out

    def extra_repr(self) -> str:
        d = self.dims
        return f"hidden={d.hidden}, heads={d.heads}, num_layers={self.num_layers}, conv={list(d.conv_dim)[:d.n_conv]}, compute_dtype={self.compute_dtype}"
