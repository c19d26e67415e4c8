#!/usr/bin/env python3
"""Dropout training fixture for tests/golden: made by running the REFERENCE on CPU (build container only).

    python tests/golden/make_golden_dropout.py

train_dropout   the reference's own EdgeDiffusionDecoder (hidden 32, 2 heads, 2 layers, dropout 0.2, synth_state_dict weights) in
                .train() under the v-prediction objective of train_v2.train_step, at B = 2, T = 24, S = 12 with the inputs of
                make_golden_train.py.  Its attention modules run their manual path (use_flash = False: softmax, self.dropout, @ v --
                the definition of F.scaled_dot_product_attention's dropout_p), and every nn.Dropout instance is replaced by a module
                that multiplies by the mask of tests/dropout_util.py for its (site, layer) and by 1 / (1 - p_eff): the reference
                decides WHERE dropout acts and how it scales, the contract of include/edtts.h decides which elements.  Recorded:
                inputs, p, seed, the loss and every parameter's gradient in fp32 ("g32.<key>") and from the same run in fp64
                ("g64.<key>", the arbiter, with the shims of make_golden_train.py).  Inputs + outputs only.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets sys.path for the reference + this repo's synth module, chdirs to a scratch dir)
from make_golden import OUT, REPO, make_decoder, npf, ref, rnd  # noqa: E402
from make_golden_train import B, S, T, T_STEPS, TimeEmb64, objective  # noqa: E402
from edge_diffusion_tts.layers import mla as ref_mla  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import dropout_util as U  # noqa: E402

CFG_KW = dict(hidden=32, heads=2, layers=2, dropout=0.2)
GEN = 20  # the fixture's seed is the first draw of torch.Generator().manual_seed(GEN): a decoder with that dropout_generator draws it
SEED = U.seeds_of(GEN)[0]


class MaskDropout(torch.nn.Module):
    """Stands where an nn.Dropout stood: in training mode x * keep(site, layer) * 1 / (1 - p_eff)."""

    def __init__(self, site, layer, p, seed):
        super().__init__()
        self.site, self.layer, self.p, self.seed = site, layer, p, seed

    def forward(self, x):
        if not self.training:  # (as nn.Dropout)
            return x
        if self.site in (U.SITE_ATTN, U.SITE_CROSS):
            b, h, tq, tk = x.shape
            keep = U.attn_keep(self.seed, self.p, self.layer, self.site, b, h, tq, tk)
        else:
            b, t, n = x.shape
            keep = U.row_keep(self.seed, self.p, self.layer, self.site, b * t, n).reshape(b, t, n)
        return x * torch.from_numpy(keep).to(x.dtype) * U.scale(self.p)


def with_masks(dec, p, seed):
    n = 0
    for l, layer in enumerate(dec.layers):
        for mod, site in ((layer.attn, U.SITE_ATTN), (layer.cross_attn, U.SITE_CROSS)):
            assert isinstance(mod.dropout, torch.nn.Dropout) and mod.dropout.p == p
            mod.use_flash = False
            mod.dropout = MaskDropout(site, l, p, seed)
        net = layer.ffn.net
        for idx, site in ((2, U.SITE_ACT), (4, U.SITE_DOWN)):
            assert isinstance(net[idx], torch.nn.Dropout) and net[idx].p == p
            net[idx] = MaskDropout(site, l, p, seed)
        n += 4
    left = [k for k, m in dec.named_modules() if isinstance(m, torch.nn.Dropout)]
    assert not left, left  # nothing else in the decoder drops
    return n


def train_dropout():
    cfg = ref.CFG(device="cpu", **CFG_KW)
    p = float(cfg.dropout)
    dec = make_decoder(cfg, seed=7)
    assert with_masks(dec, p, SEED) == 4 * cfg.layers
    dec.train()
    sch = ref.DiffusionSchedule(cfg.diff_steps)
    x0 = rnd((B, T, cfg.n_mels), 21, 0, 1.0)
    noise = rnd((B, T, cfg.n_mels), 21, 1, 1.7)
    feats = rnd((B, S, cfg.semantic_dim), 21, 2, 1.0)
    t = torch.tensor(T_STEPS)
    out = dict(x0=npf(x0), noise=npf(noise), feats=npf(feats), t=npf(t), cfg=np.array([CFG_KW["hidden"], CFG_KW["heads"], CFG_KW["layers"]]),
               p=np.float32(p), seed=np.int64(SEED), gen=np.int64(GEN))

    loss = objective(dec, sch, x0, noise, t, feats)
    loss.backward()
    out["loss32"] = np.float32(loss.item())
    for k, prm in dec.named_parameters():
        if prm.grad is not None:
            out["g32." + k] = npf(prm.grad)

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
    for k, prm in dec64.named_parameters():
        if prm.grad is not None:
            out["g64." + k] = npf(prm.grad)
            e = float(np.abs(out["g32." + k].astype(np.float64) - out["g64." + k]).max() / np.abs(out["g64." + k]).max())
            worst = max(worst, e)
    assert set(k[4:] for k in out if k.startswith("g32.")) == set(k[4:] for k in out if k.startswith("g64."))

    # the same objective with dropout off moves: the fixture is not the eval arithmetic
    dec.eval()
    loss_eval = objective(dec, sch, x0, noise, t, feats)
    print(f"train_dropout: loss {loss.item():.6f} (fp64 {loss64.item():.9f}; eval-mode loss {loss_eval.item():.6f}); "
          f"{sum(k.startswith('g32.') for k in out)} gradient tensors; worst fp32-vs-fp64 relative error {worst:.2e}")
    np.savez_compressed(os.path.join(OUT, "train_dropout.npz"), **out)


if __name__ == "__main__":
    train_dropout()
    f = os.path.join(OUT, "train_dropout.npz")
    print(f"train_dropout.npz: {os.path.getsize(f) / 1024:.0f} KiB")
