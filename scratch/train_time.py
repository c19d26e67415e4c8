#!/usr/bin/env python3
"""One training step's decoder part -- forward + backward of the v-prediction loss (train_v2.train_step) -- on
EdgeDiffusionDecoder(kernels="generic", autograd=True) against a torch-eager restatement of the decoder, same GPU, fp32.

    python scratch/train_time.py [--out profiles/train_time.json] [--reps 20] [--shapes 8x173x100,64x512x256] [--one-step ours|eager] [--ids]

Default model (hidden 160, 4 heads, 80 mels, 4 layers, window 64).  Per shape: warm-up, then `reps` timed steps of each
implementation in both orders (ours first / eager first), medians of hipEvent times; the tape size in bytes.
--one-step runs a single warmed step of one implementation and nothing else (the process to put under a kernel trace).
--ids feeds token ids instead of features (the token_emb gather and its scatter-add gradient instead of sem_proj)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "edge-diffusion-tts_amd"))
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, native, synth_state_dict  # noqa: E402

DEV = "cuda"


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps, self.weight = eps, nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight


class AdaNorm(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm, self.proj = RMSNorm(dim), nn.Linear(dim, 2 * dim)

    def forward(self, x, cond):
        scale, shift = self.proj(cond).chunk(2, dim=-1)
        return self.norm(x) * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)


class Block(nn.Module):
    def __init__(self, H, heads, ffn_mult, window):
        super().__init__()
        self.heads, self.window = heads, window
        self.norm1, self.norm2, self.norm3 = AdaNorm(H), RMSNorm(H), AdaNorm(H)
        self.qkv, self.proj = nn.Linear(H, 3 * H, bias=False), nn.Linear(H, H)
        self.q_proj, self.kv_down, self.kv_norm = nn.Linear(H, H, bias=False), nn.Linear(H, H // 2, bias=False), RMSNorm(H // 2)
        self.kv_up, self.out_proj = nn.Linear(H // 2, 2 * H, bias=False), nn.Linear(H, H, bias=False)
        self.up, self.down = nn.Linear(H, 2 * ffn_mult * H), nn.Linear(ffn_mult * H, H)

    def split(self, x):
        B, T, H = x.shape
        return x.view(B, T, self.heads, H // self.heads).transpose(1, 2)

    def forward(self, h, ctx, cond, mask):
        B, T, H = h.shape
        q, k, v = (self.split(u) for u in self.qkv(self.norm1(h, cond)).chunk(3, dim=-1))
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        h = h + self.proj(a.transpose(1, 2).reshape(B, T, H))
        q = self.split(self.q_proj(self.norm2(h)))
        k, v = (self.split(u) for u in self.kv_up(self.kv_norm(self.kv_down(ctx))).chunk(2, dim=-1))
        a = F.scaled_dot_product_attention(q, k, v)
        h = h + self.out_proj(a.transpose(1, 2).reshape(B, T, H))
        val, gate = self.up(self.norm3(h, cond)).chunk(2, dim=-1)
        return h + self.down(val * F.silu(gate))


class EagerDecoder(nn.Module):
    """Plain nn.Module restatement of the decoder (features as context), F.scaled_dot_product_attention with the band mask."""

    def __init__(self, cfg, max_len=1000, max_ctx=512):
        super().__init__()
        H = cfg.hidden
        self.H, self.window = H, cfg.attn_window_size
        self.sem_proj, self.in_proj = nn.Linear(cfg.semantic_dim, H), nn.Linear(cfg.n_mels, H)
        self.token_emb = nn.Embedding(cfg.codebook_size, H)
        self.t1, self.t3, self.step_emb = nn.Linear(H, H), nn.Linear(H, H), nn.Embedding(16, H)
        self.blocks = nn.ModuleList(Block(H, cfg.heads, cfg.ffn_mult, cfg.attn_window_size) for _ in range(cfg.layers))
        self.final_norm, self.out_proj = nn.LayerNorm(H), nn.Linear(H, cfg.n_mels)
        nn.init.normal_(self.out_proj.weight, std=0.02)
        for name, n in (("pe", max_len), ("cpe", max_ctx)):
            pos = torch.arange(n).unsqueeze(1)
            div = torch.exp(torch.arange(0, H, 2) * (-math.log(10000.0) / H))
            pe = torch.zeros(n, H)
            pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * div), torch.cos(pos * div)
            self.register_buffer(name, pe)

    def forward(self, x_t, t, sem_features, step_idx):
        half = self.H // 2
        freqs = torch.exp(torch.arange(half, device=t.device, dtype=torch.float32) * (-math.log(10000.0) / (half - 1)))
        args = t.float().unsqueeze(1) * freqs.unsqueeze(0)
        cond = self.t3(F.gelu(self.t1(torch.cat([torch.sin(args), torch.cos(args)], dim=1)))) + self.step_emb(step_idx)
        ctx = self.token_emb(sem_features) if sem_features.dtype == torch.long else self.sem_proj(sem_features)
        ctx = ctx + self.cpe[: sem_features.shape[1]]
        h = self.in_proj(x_t) + self.pe[: x_t.shape[1]]
        mask = None
        if self.window is not None:
            i = torch.arange(x_t.shape[1], device=x_t.device)
            mask = (i[None, :] - i[:, None]).abs() <= self.window
        for b in self.blocks:
            h = b(h, ctx, cond, mask)
        return self.out_proj(self.final_norm(h))


def make_step(dec, sch, cfg, B, T, S, ours, ids=False):
    g = torch.Generator().manual_seed(B + T)
    x0 = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    noise = torch.randn(B, T, cfg.n_mels, generator=g).to(DEV)
    feats = torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV)
    sem = torch.randint(0, cfg.codebook_size, (B, S), generator=g).to(DEV)
    t = torch.randint(1, 1000, (B,), generator=g).to(DEV)
    si = torch.zeros(B, dtype=torch.long, device=DEV)

    def step():
        dec.zero_grad(set_to_none=True)
        x_t, _ = sch.q_sample(x0, t, noise)
        if ids:
            v = dec(x_t, t, sem, si) if ours else dec(x_t, t, sem, si)
        else:
            v = dec(x_t, t, sem_features=feats, step_idx=si) if ours else dec(x_t, t, feats, si)
        loss = F.mse_loss(v, sch.get_v_target(x0, noise, t))
        loss.backward()
        return loss

    return step


def timed(step, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x173x100,64x512x256")
    ap.add_argument("--one-step", default=None, choices=("ours", "eager"))
    ap.add_argument("--ids", action="store_true")
    a = ap.parse_args()
    cfg = CFG(device=DEV, dropout=0.0)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    ours = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    ours.load_state_dict(synth_state_dict(cfg, 0))
    ours = ours.to(DEV).train()
    eager = EagerDecoder(cfg).to(DEV).train()
    results = []
    for shape in a.shapes.split(","):
        B, T, S = (int(v) for v in shape.split("x"))
        steps = {"ours": make_step(ours, sch, cfg, B, T, S, True, a.ids), "eager": make_step(eager, sch, cfg, B, T, S, False, a.ids)}
        if a.one_step:
            for _ in range(a.warmup):
                steps[a.one_step]()
            torch.cuda.synchronize()
            print(f"one {a.one_step} step at {shape}: loss {float(steps[a.one_step]()):.4f}")
            torch.cuda.synchronize()
            continue
        for s in steps.values():
            for _ in range(a.warmup):
                s()
        torch.cuda.synchronize()
        ms = {"ours": [], "eager": []}
        for order in (("ours", "eager"), ("eager", "ours")):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        r = dict(B=B, T=T, S=S, context="ids" if a.ids else "features", ours_ms_by_order=ms["ours"], eager_ms_by_order=ms["eager"], ours_ms=statistics.median(ms["ours"]),
                 eager_ms=statistics.median(ms["eager"]), tape_bytes=native.train_tape_bytes(ours.dims(), B, T, S),
                 scratch_bytes=native.train_scratch_bytes(ours.dims(), B, T, S))
        r["ours_over_eager"] = r["ours_ms"] / r["eager_ms"]
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        with open(a.out, "w") as f:
            json.dump(dict(model="hidden 160, heads 4, n_mels 80, layers 4, window 64, fp32", device=torch.cuda.get_device_name(0),
                           reps=a.reps, warmup=a.warmup, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
