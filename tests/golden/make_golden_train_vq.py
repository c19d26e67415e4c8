#!/usr/bin/env python3
"""VQ-training fixture for tests/golden: made by running the REFERENCE on CPU (build container only).

    python tests/golden/make_golden_train_vq.py

train_vq   the reference's own VectorQuantizer (models/vq.py; commit 0.25, decay 0.99, epsilon 1e-5, reset_unused_every = 2) behind a
           proj written as models/encoder.py:41-46 builds it -- Linear, GELU, LayerNorm, Linear --, in .train() mode, at in_dim 48,
           S = 16, K = 24, B x T = 2 x 24: THREE consecutive forwards / backwards of (z_q . C).sum() + 10 vq_loss with no optimizer
           step in between (the EMA update moves the codebook, and the second call resets the dead codes).  The reference draws
           the reset's rows with torch.randperm from the default generator: the generator is seeded before every call and the
           permutation it returns is recorded ("perm.<step>").  Recorded: the inputs, the weights (synth_semantic_head) and starting
           buffers (tests/vq_train_util.py: start_buffers), and per step idx, vq_loss, the gradient of every parameter, the three
           buffers and the codebook after the call.  The reference's _ema_update is fp32 only (its one-hot is .float()), so this is
           its fp32 run.  Inputs + outputs only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets sys.path for the reference + this repo's synth module, chdirs to a scratch dir)
from make_golden import OUT, REPO  # noqa: E402
from edge_diffusion_tts.models.vq import VectorQuantizer as RefVQ  # noqa: E402
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head  # noqa: E402

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import vq_train_util as U  # noqa: E402

IN_DIM, S, K, B, T = 48, 16, 24, 2, 24
WEIGHT_SEED, STEPS, RESET_EVERY, PERM_SEED = 7, 3, 2, 1234
FEATURE_SEEDS = range(100, 200)  # the first one at which the margin conditions of tests/vq_train_util.py hold at every step is taken


def margins(w, q_sd, x, C, perms):
    head = U.Head(w, q_sd, torch.float64, reset_unused_every=RESET_EVERY)
    gap, dead = float("inf"), float("inf")
    for s in range(STEPS):
        r = head.step(x, C, perm=lambda n, s=s: perms[s][:n])
        gap = min(gap, float(r["gap"].min()))
        if r["reset"]:
            dead = min(dead, float(r["dead_margin"]))
    return gap, dead


def main():
    proj_sd, q_sd = synth_semantic_head(IN_DIM, S, None, codebook_size=K, seed=WEIGHT_SEED)
    q_sd = dict(q_sd)
    q_sd["ema_cluster_size"], q_sd["ema_w"] = U.start_buffers(K, S, q_sd["codebook.weight"], WEIGHT_SEED)
    w = U.weights_of(proj_sd, q_sd)
    C = torch.randn(B, T, S, generator=torch.Generator().manual_seed(B * 1000 + T))
    perms = []
    for s in range(STEPS):
        torch.manual_seed(PERM_SEED + s)
        perms.append(torch.randperm(B * T))
    for fs in FEATURE_SEEDS:
        x = synth_hubert_features(B, T, IN_DIM, fs)
        gap, dead = margins(w, q_sd, x, C, perms)
        if gap >= U.MIN_GAP and dead >= U.MIN_DEAD:
            break
    else:
        raise SystemExit("no feature seed satisfies the margin conditions")
    proj = torch.nn.Sequential(torch.nn.Linear(IN_DIM, S), torch.nn.GELU(), torch.nn.LayerNorm(S), torch.nn.Linear(S, S))
    proj.load_state_dict(proj_sd)
    vq = RefVQ(S, K, commit=U.COMMIT, decay=U.DECAY, epsilon=U.EPSILON, reset_unused_every=RESET_EVERY)
    vq.load_state_dict(q_sd)
    proj.train()
    vq.train()
    out = {"dims": np.array([IN_DIM, S, K, B, T, STEPS, RESET_EVERY], np.int64), "feature_seed": np.int64(fs), "h": x.numpy(), "C": C.numpy(),
           "loss_w": np.float64(U.LOSS_W), "gap": np.float64(gap), "dead_margin": np.float64(dead)}
    out.update({"w.proj." + k: v.numpy() for k, v in proj_sd.items()})
    out.update({"w.vq." + k: v.numpy() for k, v in q_sd.items()})
    names = {"proj.0.weight": "w1", "proj.0.bias": "b1", "proj.2.weight": "lng", "proj.2.bias": "lnb", "proj.3.weight": "w3", "proj.3.bias": "b3",
             "vq.codebook.weight": "cb"}
    params = {"proj." + k: v for k, v in proj.named_parameters()}
    params.update({"vq." + k: v for k, v in vq.named_parameters()})
    for s in range(STEPS):
        for v in params.values():
            v.grad = None
        torch.manual_seed(PERM_SEED + s)
        zq, idx, loss, ppl, used = vq(proj(x))
        ((zq * C).sum() + U.LOSS_W * loss).backward()
        out[f"perm.{s}"] = perms[s].numpy()
        out[f"idx.{s}"] = idx.numpy()
        out[f"loss.{s}"] = loss.detach().numpy()
        out[f"ecs.{s}"] = vq.ema_cluster_size.detach().numpy().copy()
        out[f"ema_w.{s}"] = vq.ema_w.detach().numpy().copy()
        out[f"cb.{s}"] = vq.codebook.weight.detach().numpy().copy()
        out[f"count.{s}"] = np.int64(int(vq.update_count))
        for n, k in names.items():
            out[f"g.{k}.{s}"] = params[n].grad.numpy().copy()
    print(f"train_vq: feature seed {fs}, gap {gap:.2e}, reset margin {dead:.2e}; losses {[float(out[f'loss.{s}']) for s in range(STEPS)]}; "
          f"distinct ids {[len(np.unique(out[f'idx.{s}'])) for s in range(STEPS)]}")
    np.savez_compressed(os.path.join(OUT, "train_vq.npz"), **out)


if __name__ == "__main__":
    main()
