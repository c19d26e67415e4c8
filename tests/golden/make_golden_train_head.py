#!/usr/bin/env python3
"""Head-training fixture for tests/golden: made by running the REFERENCE on CPU (build container only).

    python tests/golden/make_golden_train_head.py

train_head   the reference's own FSQEncoder (models/fsq.py) behind a proj written as train_v2.py:54-60 builds it -- Linear, GELU,
             LayerNorm, Dropout, Linear -- whose Dropout is replaced by a module that applies the mask contract's head site
             (tests/sem_train_util.py: stream word 0x40000), feeding the reference's own EdgeDiffusionDecoder (hidden 32, 2 heads,
             2 layers, dropout 0, semantic_dim 16; the head's in_dim is 48) through sem_features under the v-prediction objective of
             train_v2.train_step at B = 2, T = 24, S = 12, with the decoder inputs of make_golden_train.py.  Recorded: the inputs, the
             head's weights (synth_semantic_head), p, the seed, idx, the loss and the gradient of every decoder, proj and FSQEncoder
             parameter after ONE loss.backward(), in fp32 ("g32.<key>") and from the same run in fp64 ("g64.<key>", the arbiter, with
             the shims of make_golden_train.py).  Inputs + outputs only.
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets sys.path for the reference + this repo's synth module, chdirs to a scratch dir)
from make_golden import OUT, REPO, make_decoder, npf, ref, rnd  # noqa: E402
from make_golden_train import B, S, T, T_STEPS, TimeEmb64  # noqa: E402
from edge_diffusion_tts.layers import mla as ref_mla  # noqa: E402
from edge_diffusion_tts.models.fsq import FSQEncoder as RefFSQEncoder  # noqa: E402
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import dropout_util as DU  # noqa: E402
import sem_train_util as U  # noqa: E402

CFG_KW = dict(hidden=32, heads=2, layers=2, dropout=0.0, semantic_dim=16)
IN_DIM, LEVELS, P = 48, [8, 6, 5, 5, 5], 0.2
GEN = 30  # the fixture's seed is the first draw of torch.Generator().manual_seed(GEN)
SEED = DU.seeds_of(GEN)[0]
FEATURE_SEEDS = range(40, 140)  # the first one at which every FSQ decision has an fp64 margin >= 1e-4 is taken


class MaskDropout(torch.nn.Module):
    """Stands where proj's nn.Dropout stood: in training mode x * keep * 1 / (1 - p_eff) with the head site's mask."""

    def __init__(self, p, seed):
        super().__init__()
        self.p, self.seed = p, seed

    def forward(self, x):
        if not self.training:
            return x
        b, t, n = x.shape
        return x * U.head_multiplier(self.seed, self.p, b, t, n, x.dtype)


class Head(torch.nn.Module):
    def __init__(self, sem_dim):
        super().__init__()
        self.proj = torch.nn.Sequential(torch.nn.Linear(IN_DIM, sem_dim), torch.nn.GELU(), torch.nn.LayerNorm(sem_dim), torch.nn.Dropout(P),
                                        torch.nn.Linear(sem_dim, sem_dim))  # train_v2.py:54-60
        self.fsq = RefFSQEncoder(sem_dim, LEVELS)

    def forward(self, h):
        return self.fsq(self.proj(h.detach()))  # train_v2.py:74-78


def objective(head, dec, sch, x0, noise, t, h):
    z_q, idx, _, _, _ = head(h)
    x_t, _ = sch.q_sample(x0, t, noise)
    v_pred = dec(x_t, t, sem_features=z_q, step_idx=torch.zeros(B, dtype=torch.long))
    return F.mse_loss(v_pred, sch.get_v_target(x0, noise, t)), idx


def train_head():
    cfg = ref.CFG(device="cpu", **CFG_KW)
    dec = make_decoder(cfg, seed=7).train()
    proj_sd, q_sd = synth_semantic_head(IN_DIM, cfg.semantic_dim, LEVELS, seed=9, dropout_layout=True)
    head = Head(cfg.semantic_dim)
    head.proj.load_state_dict(proj_sd)
    head.fsq.load_state_dict(q_sd)
    assert isinstance(head.proj[3], torch.nn.Dropout)
    head.proj[3] = MaskDropout(P, SEED)
    head.train()
    sch = ref.DiffusionSchedule(cfg.diff_steps)
    x0 = rnd((B, T, cfg.n_mels), 21, 0, 1.0)
    noise = rnd((B, T, cfg.n_mels), 21, 1, 1.7)
    t = torch.tensor(T_STEPS)

    head64, dec64 = copy.deepcopy(head).double(), copy.deepcopy(dec).double()
    dec64.time_emb[0] = TimeEmb64(dec64.time_emb[0].dim)
    for fs in FEATURE_SEEDS:
        h = synth_hubert_features(B, S, IN_DIM, fs)
        with torch.no_grad():
            zb = torch.tanh(head64.fsq.proj_down(head64.proj(h.double())))
            idx64, idx32 = head64(h.double())[1], head(h)[1]
        if float(U.margin_of(zb, LEVELS).min()) >= U.MIN_MARGIN and torch.equal(idx64, idx32):
            break
    else:
        raise SystemExit("no feature seed satisfies the margin condition")

    out = dict(x0=npf(x0), noise=npf(noise), h=npf(h), t=npf(t), p=np.float32(P), seed=np.int64(SEED), gen=np.int64(GEN),
               cfg=np.array([CFG_KW["hidden"], CFG_KW["heads"], CFG_KW["layers"], CFG_KW["semantic_dim"], IN_DIM]),
               levels=np.array(LEVELS, dtype=np.int64), feature_seed=np.int64(fs), margin=np.float64(float(U.margin_of(zb, LEVELS).min())))
    out.update({"w.proj." + k: npf(v) for k, v in proj_sd.items()})
    out.update({"w.fsq." + k: npf(v) for k, v in q_sd.items()})

    def named(hd, dc):
        yield from (("decoder." + k, p) for k, p in dc.named_parameters())
        yield from (("encoder.proj." + k, p) for k, p in hd.proj.named_parameters())
        yield from (("encoder.fsq." + k, p) for k, p in hd.fsq.named_parameters())

    loss, idx = objective(head, dec, sch, x0, noise, t, h)
    loss.backward()
    out["loss32"], out["idx"] = np.float32(loss.item()), npf(idx)
    for k, p in named(head, dec):
        if p.grad is not None:
            out["g32." + k] = npf(p.grad)

    real_forward = ref_mla.RMSNorm.forward
    ref_mla.RMSNorm.forward = lambda self, x: self._norm(x) * self.weight
    try:
        sch64 = ref.DiffusionSchedule(cfg.diff_steps)
        for n, v in list(vars(sch64).items()):
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(sch64, n, v.double())
        loss64, idx64 = objective(head64, dec64, sch64, x0.double(), noise.double(), t, h.double())
        loss64.backward()
    finally:
        ref_mla.RMSNorm.forward = real_forward
    assert torch.equal(idx64, idx)
    out["loss64"] = np.float64(loss64.item())
    worst = 0.0
    for k, p in named(head64, dec64):
        if p.grad is not None:
            out["g64." + k] = npf(p.grad)
            e = float(np.abs(out["g32." + k].astype(np.float64) - out["g64." + k]).max() / np.abs(out["g64." + k]).max())
            worst = max(worst, e)
    assert set(k[4:] for k in out if k.startswith("g32.")) == set(k[4:] for k in out if k.startswith("g64."))
    assert sum(k.startswith("g64.encoder.") for k in out) == 10
    head.eval()
    loss_eval, _ = objective(head, dec, sch, x0, noise, t, h)
    print(f"train_head: feature seed {fs}, margin {float(out['margin']):.2e}, {len(np.unique(out['idx']))} distinct ids; loss {loss.item():.6f} "
          f"(fp64 {loss64.item():.9f}; with the head in eval mode {loss_eval.item():.6f}); {sum(k.startswith('g32.') for k in out)} gradient "
          f"tensors; worst fp32-vs-fp64 relative error {worst:.2e}")
    np.savez_compressed(os.path.join(OUT, "train_head.npz"), **out)


if __name__ == "__main__":
    train_head()
    f = os.path.join(OUT, "train_head.npz")
    print(f"train_head.npz: {os.path.getsize(f) / 1024:.0f} KiB")
