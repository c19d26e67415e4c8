"""Shared by tests/test_attn_bf16_host.py and tests/test_attn_bf16_gpu.py: the model of bf16 attention
(EdgeDiffusionDecoder(kernels="generic", attn_dtype="bf16")), two more cases for attention geometry that
train_util's G1-G5 do not reach, and the yardsticks.  The bars, the error measures and the autocast run A are tests/train_bf16_util.py's
own (imported, not restated): A already rounds both attention contractions, so it is the yardstick of this option too.

  M_attn  oracle.edtts_oracle.attention (and dropout_util._attention, with its `mult`) replaced, for a run's duration, by an autograd
          function that implements the rounding contract of include/edtts.h, EDTTS_ATTN_BF16:
            forward   S = bf16(q) bf16(k)^T / sqrt(d); mask, maximum, exp and the row sum l in the run's dtype from the unrounded
                      probabilities; O = bf16(P~ o D) bf16(v) / l   (P~ = exp(S - max), D = the dropout multiplier or 1)
            backward  delta = rowsum(dO o O) unrounded; dP = bf16(dO) bf16(v)^T; P = P~ / l unrounded; dV = bf16(P o D)^T bf16(dO);
                      dS = P o (D o dP - delta); dQ = bf16(dS) bf16(k) / sqrt(d); dK = bf16(dS)^T bf16(q) / sqrt(d)
  model("attn")  M_attn alone; model("both"): stacked with train_bf16_util.model(), the bf16 linears.
The kernels are another draw of the same rounding noise (an online softmax, another summation order) and are never compared with M
element by element.  Every run is computed once per (case, variant) and never modified."""
import contextlib
import functools
from unittest import mock

import torch

import dropout_util
import train_bf16_util as U
import train_ragged_util
import train_util
from edge_diffusion_tts_amd import CFG, synth_state_dict
from oracle import edtts_oracle as O
from train_bf16_util import (GRAD_MARGIN, MAX_MARGIN, MEDIAN_MARGIN, RMS_MARGIN, _bf16, _grad_yardsticks,  # noqa: F401
                             check_grads, check_output)

_linear_model = U.model  # (bound here: _with_model below replaces the module attribute for a call's duration)
VARIANTS = ("attn", "both")  # what M rounds: the attention contractions alone / those and every linear

# (cfg keywords, B, T, S, features, step_idx) as train_util.CASES
ACASES = {
    # one 32-wide k-step per head; the band (41 keys) crosses several 32-key steps and several 64-query blocks; T, S not multiples of 32
    "A1": (dict(hidden=64, heads=2, attn_window_size=20, layers=1), 2, 200, 70, True, True),
    # a band narrower than a tile, a context shorter than one tile, head_dim 16 (half a k-step), ids
    "A2": (dict(hidden=48, heads=3, attn_window_size=1, layers=1, codebook_size=16), 2, 37, 5, False, False),
}


@functools.lru_cache(maxsize=None)
def case(name, device="cpu"):
    """train_util.case for its own names; A1 / A2 by the same recipe."""
    if name in train_util.CASES:
        return train_util.case(name, device)
    kw, B, T, S, feats, with_step = ACASES[name]
    cfg = CFG(device=device, **kw)
    sd = synth_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(B * 1000 + T)
    inp = dict(
        x=torch.randn(B, T, cfg.n_mels, generator=g),
        t=torch.randint(0, 1000, (B,), generator=g),
        t2=torch.randint(0, 1000, (B,), generator=g),
        si=torch.randint(0, 16, (B,), generator=g) if with_step else None,
        sem=None if feats else torch.randint(0, cfg.codebook_size, (B, S), generator=g),
        f=torch.randn(B, S, cfg.semantic_dim, generator=g) if feats else None,
        target=torch.randn(B, T, cfg.n_mels, generator=g),
        target2=torch.randn(B, T, cfg.n_mels, generator=g),
    )
    return cfg, sd, inp


def shape(name):
    """(B, T, S) of a case."""
    return (train_util.CASES.get(name) or ACASES[name])[1:4]


class _Bf16Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, mult):
        scale = q.shape[-1] ** -0.5
        qb, kb, vb = _bf16(q), _bf16(k), _bf16(v)
        s = (qb @ kb.transpose(-1, -2)) * scale  # the product of two bf16 values is exact in fp32: only the operands are rounded
        if mask is not None:
            s = s.masked_fill(~mask, float("-inf"))
        pt = torch.exp(s - s.amax(dim=-1, keepdim=True))
        l = pt.sum(dim=-1, keepdim=True)  # from the unrounded probabilities
        o = (_bf16(pt if mult is None else pt * mult) @ vb) / l
        ctx.save_for_backward(qb, kb, vb, pt / l, o)
        ctx.mult, ctx.scale = mult, scale
        return o

    @staticmethod
    def backward(ctx, do):
        qb, kb, vb, p, o = ctx.saved_tensors
        mult = ctx.mult
        dob = _bf16(do)
        delta = (do * o).sum(dim=-1, keepdim=True)  # unrounded
        dp = dob @ vb.transpose(-1, -2)
        dv = _bf16(p if mult is None else p * mult).transpose(-1, -2) @ dob
        ds = p * ((dp if mult is None else dp * mult) - delta)
        dsb = _bf16(ds)
        return (dsb @ kb) * ctx.scale, (dsb.transpose(-1, -2) @ qb) * ctx.scale, dv, None, None


def model_attention(q, k, v, mask, mult=None):
    return _Bf16Attention.apply(q, k, v, mask, mult)


@contextlib.contextmanager
def model(variant="attn"):
    """The oracle's `attention` (and the masked oracle's) is M_attn for the duration; "both": its `linear` is the bf16 model's too."""
    assert variant in VARIANTS
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(O, "attention", model_attention))
        st.enter_context(mock.patch.object(dropout_util, "_attention", model_attention))
        if variant == "both":
            st.enter_context(_linear_model())
        yield


def _with_model(variant, fn, *args):
    """fn(*args) of train_bf16_util with its M replaced by this module's: A and the bars stay that module's."""
    with mock.patch.object(U, "model", functools.partial(model, variant)):
        return fn(*args)


@functools.lru_cache(maxsize=None)
def grad_yardsticks(name, two=False, variant="attn"):
    cfg, sd, inp = case(name)
    g64 = train_util.oracle_pair(name, two)[0] if name in train_util.CASES else train_util.oracle_grads(cfg, sd, inp, torch.float64, two)[1]
    return _with_model(variant, _grad_yardsticks, g64, lambda: train_util.oracle_grads(cfg, sd, inp, torch.float32, two)[1])


@functools.lru_cache(maxsize=None)
def ragged_yardsticks(variant="attn", name=U.RAGGED_CASE):
    cfg, sd, inp, t_len, s_len = train_ragged_util.case(name)
    return _with_model(variant, _grad_yardsticks, train_ragged_util.ragged_pair(name)[0],
                       lambda: train_ragged_util.ragged_grads(cfg, sd, inp, t_len, s_len, torch.float32)[1])


@functools.lru_cache(maxsize=None)
def dropout_yardsticks(variant="both", name=U.DROP_CASE):
    cfg, sd, inp = case(name)
    return _with_model(variant, _grad_yardsticks, dropout_util.oracle_pair(name, U.DROP_P, U.drop_seeds())[0],
                       lambda: dropout_util.oracle_grads(cfg, sd, inp, torch.float32, U.DROP_P, U.drop_seeds())[1])


@functools.lru_cache(maxsize=None)
def forward_yardsticks(name, variant="attn"):
    """{ref (fp64 eps), a_rms, a_max, out_m} of one decoder forward."""
    cfg, sd, inp = case(name)

    def run(dtype):
        x, f = inp["x"].to(dtype), None if inp["f"] is None else inp["f"].to(dtype)
        return O.decoder_forward(O.cast_sd(sd, dtype), x, inp["t"], inp["sem"], inp["si"], f, heads=cfg.heads, window=cfg.attn_window_size)

    return _with_model(variant, U._out_yardsticks, run)


@functools.lru_cache(maxsize=None)
def sampler_yardsticks(name, variant="attn"):
    """... of oracle.dpmpp_sample, order 2, train_bf16_util.SAMPLER_STEPS steps, on the case's x and features."""
    cfg, sd, _ = case(name)
    x_T, f = U.sampler_inputs(name)

    def run(dtype):
        return O.dpmpp_sample(O.cast_sd(sd, dtype), O.schedule_tables(cfg.diff_steps, dtype), x_T.to(dtype), f.to(dtype), U.SAMPLER_STEPS,
                              order=2, heads=cfg.heads, window=cfg.attn_window_size)

    return _with_model(variant, U._out_yardsticks, run)
