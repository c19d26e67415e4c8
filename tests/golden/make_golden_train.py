#!/usr/bin/env python3
"""Training fixture for tests/golden: made by running the REFERENCE on CPU (build container only).

    python tests/golden/make_golden_train.py

train_grads   the reference's own EdgeDiffusionDecoder (hidden 32, 2 heads, 2 layers, dropout 0, synth_state_dict weights) under the
              v-prediction objective of train_v2.train_step -- q_sample, decoder(x_t, t, sem_features=..., step_idx=0),
              mse_loss(v_pred, get_v_target) -- at B = 2, T = 24, S = 12 with fixed inputs and noise: the loss and every parameter's
              gradient after loss.backward(), in fp32 ("g32.<key>") and from the same run in fp64 ("g64.<key>", the arbiter: a deep
              copy cast to double with the two shims of SURVEY.md section 6 -- the time embedding's trig evaluated in fp64 on its
              fp32 frequencies, RMSNorm without its .float() -- and double schedule tables).  Inputs + outputs only.
"""
import copy
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets sys.path for the reference + this repo's synth module, chdirs to a scratch dir)
from make_golden import OUT, make_decoder, npf, ref, rnd  # noqa: E402
from edge_diffusion_tts.layers import mla as ref_mla  # noqa: E402

CFG_KW = dict(hidden=32, heads=2, layers=2, dropout=0.0)
B, T, S = 2, 24, 12
T_STEPS = [700, 42]


class TimeEmb64(torch.nn.Module):
    """fp64 shim for time_emb[0]: the fp32 frequencies of layers/embeddings.py:38-41, the product and the trig in fp64."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, t):
        half = self.dim // 2
        freqs = torch.exp(torch.arange(half, dtype=torch.float32) * (-math.log(10000.0) / (half - 1))).double()
        args = t.double().unsqueeze(1) * freqs.unsqueeze(0)
        return torch.cat([torch.sin(args), torch.cos(args)], dim=1)


def objective(dec, sch, x0, noise, t, feats):
    x_t, _ = sch.q_sample(x0, t, noise)
    v_pred = dec(x_t, t, sem_features=feats, step_idx=torch.zeros(B, dtype=torch.long))
    return F.mse_loss(v_pred, sch.get_v_target(x0, noise, t))


def train_grads():
    cfg = ref.CFG(device="cpu", **CFG_KW)
    dec = make_decoder(cfg, seed=7).train()  # dropout 0: training mode is the eval arithmetic
    sch = ref.DiffusionSchedule(cfg.diff_steps)
    x0 = rnd((B, T, cfg.n_mels), 21, 0, 1.0)
    noise = rnd((B, T, cfg.n_mels), 21, 1, 1.7)
    feats = rnd((B, S, cfg.semantic_dim), 21, 2, 1.0)
    t = torch.tensor(T_STEPS)
    out = dict(x0=npf(x0), noise=npf(noise), feats=npf(feats), t=npf(t), cfg=np.array([CFG_KW["hidden"], CFG_KW["heads"], CFG_KW["layers"]]))

    loss = objective(dec, sch, x0, noise, t, feats)
    loss.backward()
    out["loss32"] = np.float32(loss.item())
    for k, p in dec.named_parameters():
        if p.grad is not None:
            out["g32." + k] = npf(p.grad)

    dec64 = copy.deepcopy(dec).double()
    dec64.zero_grad(set_to_none=True)
    dec64.time_emb[0] = TimeEmb64(dec64.time_emb[0].dim)
    real_forward = ref_mla.RMSNorm.forward
    ref_mla.RMSNorm.forward = lambda self, x: self._norm(x) * self.weight
    try:
        sch64 = ref.DiffusionSchedule(cfg.diff_steps)
        for n, v in list(vars(sch64).items()):
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(sch64, n, v.double())
        loss64 = objective(dec64, sch64, x0.double(), noise.double(), t, feats.double())
        loss64.backward()
    finally:
        ref_mla.RMSNorm.forward = real_forward
    out["loss64"] = np.float64(loss64.item())
    worst = 0.0
    for k, p in dec64.named_parameters():
        if p.grad is not None:
            out["g64." + k] = npf(p.grad)
            e = float(np.abs(out["g32." + k].astype(np.float64) - out["g64." + k]).max() / np.abs(out["g64." + k]).max())
            worst = max(worst, e)
    assert set(k[4:] for k in out if k.startswith("g32.")) == set(k[4:] for k in out if k.startswith("g64."))
    print(f"train_grads: loss {loss.item():.6f} (fp64 {loss64.item():.9f}); {sum(k.startswith('g32.') for k in out)} gradient tensors; "
          f"worst fp32-vs-fp64 relative error {worst:.2e}")
    np.savez_compressed(os.path.join(OUT, "train_grads.npz"), **out)


if __name__ == "__main__":
    train_grads()
    f = os.path.join(OUT, "train_grads.npz")
    print(f"train_grads.npz: {os.path.getsize(f) / 1024:.0f} KiB")
