"""Shared by tests/test_tape_bf16_host.py and tests/test_tape_bf16_gpu.py: EdgeDiffusionDecoder(kernels="generic",
matmul_dtype="bf16", attn_dtype="bf16", tape_dtype="bf16"), DESIGN.md section 28.  The option stores four per-layer activations as
bf16 that, with both other options on, are read only by loaders that round to bf16; rounding to nearest even is idempotent, so the
bar of every comparison is bitwise equality with the same decoder at tape_dtype="f32" -- there is no tolerance anywhere in these
files.  The cases are train_util's G1-G5 and attn_bf16_util's A1 / A2 (imported, not restated)."""
import contextlib
from unittest import mock

import torch

import attn_bf16_util as AU
from edge_diffusion_tts_amd import native
from oracle import edtts_oracle as O
from train_util import CASES

NAMES = list(CASES) + ["A1", "A2"]
NARROWED = ("kv", "qkv", "qc", "act")  # the TapeLayer members that hold bf16 with the option
BOTH = native.EDTTS_MATMUL_BF16 | native.EDTTS_ATTN_BF16
BIT = native.EDTTS_TAPE_BF16


def region_shape(cfg, B, T, S, which):
    """(rows, elements per row) of a tape member, per-layer or whole-model (include/edtts.h: edtts_train_tape_region)."""
    H = cfg.hidden
    if which in native.TAPE_GLOBALS:
        return {"cond": (B * cfg.layers * 2, 2 * H), "tcond": (B, H), "ctx": (B * S, H), "hl": (B * T, H)}[which]
    return {"crp": (B * S, H // 2), "kv": (B * S, 2 * H), "h0": (B * T, H), "h1": (B * T, H), "h2": (B * T, H), "qkv": (B * T, 3 * H),
            "att1": (B * T, H), "lse1": (B * cfg.heads, T), "qc": (B * T, H), "att2": (B * T, H), "lse2": (B * cfg.heads, T),
            "act": (B * T, cfg.ffn_mult * H)}[which]


def narrowed_elements(cfg, B, T, S):
    """Elements per layer of the four narrowed regions: M 3H + M H + M FM H + B S 2H."""
    return sum(r * c for r, c in (region_shape(cfg, B, T, S, w) for w in NARROWED))


def tape_region(tape, dims, cfg, B, T, S, layer, which):
    """One member of a filled tape (a uint8 tensor) as a [rows][pitch] tensor of its element type (a view)."""
    off, n, eb = native.train_tape_region(dims, B, T, S, layer, which)
    rows, cols = region_shape(cfg, B, T, S, which)
    assert n == rows * cols * eb
    return tape[off:off + n].view(torch.bfloat16 if eb == 2 else torch.float32).view(rows, cols)


class _Stored(torch.autograd.Function):
    """What a bf16 buffer does to a value on its way from its producer to its consumers: the consumers see bf16(x); the gradient of x
    is whatever the consumers hand back (the backward never differentiates the store)."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


@contextlib.contextmanager
def stored_model(cfg, counts):
    """attn_bf16_util.model("both") with, in addition, q, k, v of both attentions and the SwiGLU output passed through _Stored before
    their consumers see them.  counts["attn"] / counts["act"]: how often each hook fired."""
    H, FH = cfg.hidden, cfg.ffn_mult * cfg.hidden
    assert FH != H  # (the down projection is told from the other linears by its input width)
    with AU.model("both"):
        attention, linear = O.attention, O.linear

        def attention_stored(q, k, v, mask, *a):
            counts["attn"] = counts.get("attn", 0) + 1
            return attention(_Stored.apply(q), _Stored.apply(k), _Stored.apply(v), mask, *a)

        def linear_stored(x, w, b=None):
            if tuple(w.shape) == (H, FH):  # ffn.net.3: its input is the SwiGLU output
                counts["act"] = counts.get("act", 0) + 1
                x = _Stored.apply(x)
            return linear(x, w, b)

        with mock.patch.object(O, "attention", attention_stored), mock.patch.object(O, "linear", linear_stored):
            yield
