#!/usr/bin/env python3
"""One training step's VQ-head part -- forward + EMA update + backward of 0.1 vq_loss, as train.py's phase 1 forms it (its decoder is
fed tokens, so z_q gets no gradient) -- on SemanticEncoder(autograd=True, train_vq=True), next to the same head in plain torch
(tests/vq_train_util.py's restatement as a module: proj, the distance matrix, argmin, the two mse losses, the one-hot EMA update) in
fp32 on the same GPU, and the EMA update's kernels alone (edtts_sem_vq_ema_update: the per-code sums of z, the slab sum, the finish).

    python scratch/vq_train_time.py [--out FILE.json] [--reps 30] [--shape 64x500] [--codes 512]

Event-timed medians of warmed steps, each variant measured in both orders; the per-kernel figures come from one torch.profiler trace
of three further steps (kernel names containing k_sem / k_bwd)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get("EDTTS_PKG_ROOT", os.path.join(REPO, "edge-diffusion-tts_amd")))
sys.path.insert(0, HERE)
from edge_diffusion_tts_amd import CFG, native  # noqa: E402
from edge_diffusion_tts_amd.encoder import SemanticEncoder  # noqa: E402
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head  # noqa: E402
from train_time import timed  # noqa: E402

DEV = "cuda"
IN_DIM, S = 768, 128


class EagerHead(nn.Module):
    """proj -> VectorQuantizer.forward in training mode (models/vq.py's operations, the reset left out: no step here resets)."""

    def __init__(self, proj_sd, q_sd, commit=0.25, decay=0.99, epsilon=1e-5):
        super().__init__()
        self.proj = nn.Sequential(nn.Linear(IN_DIM, S), nn.GELU(), nn.LayerNorm(S), nn.Linear(S, S))
        self.proj.load_state_dict(proj_sd)
        self.codebook = nn.Parameter(q_sd["codebook.weight"].clone())
        self.register_buffer("ecs", q_sd["ema_cluster_size"].clone())
        self.register_buffer("ema_w", q_sd["ema_w"].clone())
        self.commit, self.decay, self.epsilon = commit, decay, epsilon

    def forward(self, h):
        z = self.proj(h)
        flat = z.reshape(-1, S)
        C = self.codebook
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ C.t() + C.pow(2).sum(1, keepdim=True).t()
        idx = dist.argmin(dim=1)
        c = C[idx].view_as(z)
        loss = F.mse_loss(c, z.detach()) + self.commit * F.mse_loss(c.detach(), z)
        with torch.no_grad():
            enc = F.one_hot(idx, C.shape[0]).float()
            self.ecs.mul_(self.decay).add_(enc.sum(0), alpha=1 - self.decay)
            self.ema_w.mul_(self.decay).add_(enc.t() @ flat, alpha=1 - self.decay)
            C.data.copy_(self.ema_w / self.ecs.clamp_min(self.epsilon).unsqueeze(1))
        return z + (c - z).detach(), idx, loss


def kernel_times(step, n=3):
    """{kernel name: mean microseconds per step} of the library's kernels, from one profiler trace (None if the profiler is missing)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                step()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "k_sem" in e.key or "k_bwd" in e.key:
                t = getattr(e, "device_time_total", None)
                t = e.cuda_time_total if t is None else t
                out[e.key.split("(")[0]] = round(t / n, 2)
        return out
    except Exception as e:  # noqa: BLE001  (a measurement aid: the event-timed figures stand without it)
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="64x500")
    ap.add_argument("--codes", type=int, default=512)
    a = ap.parse_args()
    B, T = (int(v) for v in a.shape.split("x"))
    K = a.codes
    proj_sd, q_sd = synth_semantic_head(IN_DIM, S, None, codebook_size=K, seed=1)
    h = synth_hubert_features(B, T, IN_DIM, 101).to(DEV)
    cfg = CFG(device=DEV, use_fsq=False, codebook_size=K, semantic_dim=S, vq_commit=0.25, dropout=0.0)
    enc = SemanticEncoder(cfg, in_dim=IN_DIM, autograd=True, train_vq=True)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    enc = enc.to(DEV).train()
    eager = EagerHead(proj_sd, q_sd).to(DEV).train()

    def ours():
        enc.zero_grad(set_to_none=True)
        loss = enc.forward_features(h)[2]
        (0.1 * loss).backward()
        return loss

    def ours_forward():
        with torch.no_grad():
            return enc.encode_features(h)

    def plain():
        eager.zero_grad(set_to_none=True)
        loss = eager(h)[2]
        (0.1 * loss).backward()
        return loss

    dims = enc._dims()
    with torch.no_grad():
        idx, z, _, counts = native.sem_encode(dims, enc._pack.get(dims, enc._slots()), h, want_z=True)
    ecs, ema_w, cb = enc.vq.ema_cluster_size.clone(), enc.vq.ema_w.clone(), enc.vq.codebook.weight.detach().clone()

    def ema_alone():
        native.sem_vq_ema_update(dims, idx, z, None, counts, 0.99, 1e-5, ecs, ema_w, cb)

    steps = {"ours_step": ours, "eager_step": plain, "ours_inference_forward": ours_forward, "ours_ema_update": ema_alone}
    for s in steps.values():
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for order in (list(steps), list(steps)[::-1]):
        for k in order:
            ms[k].append(statistics.median(timed(steps[k], a.reps)))
    r = dict(B=B, T=T, K=K, S=S, in_dim=IN_DIM, **{k + "_ms_by_order": v for k, v in ms.items()},
             **{k + "_ms": statistics.median(v) for k, v in ms.items()}, kernels_us=kernel_times(ours))
    print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup, result=r), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
