#!/usr/bin/env python3
"""Forward + backward of the semantic head -- proj (Linear, GELU, LayerNorm, Dropout, Linear) and FSQEncoder, the part of
train_v2.train_step that SemanticEncoder(autograd=True) runs -- against a torch-eager composition of the same head, same GPU, fp32.

    python scratch/sem_train_time.py [--out profiles/sem_train_time.json] [--reps 20] [--shapes 8x150,64x500] [--one-step ours|eager]
                                     [--kernel-stats FILE.csv ...]

Default head: 768 -> 128, levels [4,4,3,3,2,2,2,2], dropout off (.eval(): the masks cost one Philox draw per four elements and are
not what is compared).  Per shape (B x T_feat frames): warm-up, then `reps` timed steps of each implementation in both orders,
medians of hipEvent times; the tape and scratch sizes.  --one-step runs a single warmed step of one implementation and nothing else
(the process to put under a kernel trace); --kernel-stats folds the trace's kernel-stats CSV files (label=path) into the JSON."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("EDTTS_PKG_ROOT", os.path.join(REPO, "edge-diffusion-tts_amd")))
from edge_diffusion_tts_amd import CFG, native  # noqa: E402
from edge_diffusion_tts_amd.encoder import SemanticEncoder  # noqa: E402
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head  # noqa: E402

DEV = "cuda"
IN_DIM, S, LEVELS = 768, 128, [4, 4, 3, 3, 2, 2, 2, 2]


class EagerHead(nn.Module):
    """train_v2.py:54-78 in plain torch: proj, then FSQEncoder with FSQ's straight-through line."""

    def __init__(self):
        super().__init__()
        self.proj = nn.Sequential(nn.Linear(IN_DIM, S), nn.GELU(), nn.LayerNorm(S), nn.Dropout(0.0), nn.Linear(S, S))
        self.proj_down, self.proj_up = nn.Linear(S, len(LEVELS)), nn.Linear(len(LEVELS), S)
        lv = torch.tensor(LEVELS, dtype=torch.float32)
        self.register_buffer("half_lv", (lv - 1) / 2)  # ("half" is a method of nn.Module)
        self.register_buffer("top", lv - 1)
        self.register_buffer("basis", torch.cumprod(torch.tensor([1] + LEVELS[:-1]), 0))

    def forward(self, h):
        zb = torch.tanh(self.proj_down(self.proj(h)))
        q = torch.minimum(torch.clamp(torch.round((zb + 1) * self.half_lv), min=0), self.top) / self.half_lv - 1
        zq_low = zb + (q - zb).detach()
        idx = (((zq_low + 1) * self.half_lv).round().long() * self.basis).sum(-1)
        return self.proj_up(zq_low), idx


def make_step(mod, B, T, ours):
    h = synth_hubert_features(B, T, IN_DIM, 1).to(DEV)
    C = torch.randn(B, T, S, generator=torch.Generator().manual_seed(B + T)).to(DEV)

    def step():
        mod.zero_grad(set_to_none=True)
        zq = mod.quantize_features(h)[0] if ours else mod(h)[0]
        loss = (zq * C).sum()
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


def kernel_stats(path, top=12):
    """rocprofv3 --kernel-trace --stats: the kernel_stats CSV -> [{name, calls, total_us, pct}] of the largest entries"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    out = [dict(name=r["Name"][:100], calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3, pct=float(r["Percentage"])) for r in rows]
    return sorted(out, key=lambda r: -r["total_us"])[:top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="8x150,64x500")
    ap.add_argument("--one-step", default=None, choices=("ours", "eager"))
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    cfg = CFG(device=DEV, use_fsq=True, fsq_levels=LEVELS, semantic_dim=S, dropout=0.0)
    ours = SemanticEncoder(cfg, in_dim=IN_DIM, proj_dropout=True, autograd=True)
    proj_sd, q_sd = synth_semantic_head(IN_DIM, S, LEVELS, seed=1, dropout_layout=True)
    ours.proj.load_state_dict(proj_sd)
    ours.vq.load_state_dict(q_sd)
    ours = ours.to(DEV).eval()
    eager = EagerHead()
    eager.proj.load_state_dict(proj_sd)
    eager.proj_down.load_state_dict({k[len("proj_down."):]: v for k, v in q_sd.items() if k.startswith("proj_down.")})
    eager.proj_up.load_state_dict({k[len("proj_up."):]: v for k, v in q_sd.items() if k.startswith("proj_up.")})
    eager = eager.to(DEV).eval()
    results = []
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        steps = {"ours": make_step(ours, B, T, True), "eager": make_step(eager, B, T, False)}
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
        # the two implementations compute the same thing
        go = {k: v.grad.clone() for k, v in ours.proj.named_parameters()}
        steps["eager"]()
        worst = max(float((go[k] - v.grad).abs().max() / v.grad.abs().max()) for k, v in eager.proj.named_parameters())
        ms = {"ours": [], "eager": []}
        for order in (("ours", "eager"), ("eager", "ours")):
            for k in order:
                ms[k].append(statistics.median(timed(steps[k], a.reps)))
        dims = ours._dims()
        r = dict(B=B, T=T, frames=B * T, ours_ms_by_order=ms["ours"], eager_ms_by_order=ms["eager"], ours_ms=statistics.median(ms["ours"]),
                 eager_ms=statistics.median(ms["eager"]), proj_grad_worst_rel_diff=worst, tape_bytes=native.sem_train_tape_bytes(dims, B, T),
                 scratch_bytes=native.sem_train_scratch_bytes(dims, B, T))
        r["ours_over_eager"] = r["ours_ms"] / r["eager_ms"]
        print(json.dumps(r))
        results.append(r)
    if a.out and results:
        doc = dict(head=f"{IN_DIM} -> {S}, levels {LEVELS}, fp32, dropout off", device=torch.cuda.get_device_name(0), reps=a.reps,
                   warmup=a.warmup, results=results)
        if a.kernel_stats:
            doc["kernel_trace"] = {item.split("=", 1)[0]: kernel_stats(item.split("=", 1)[1]) for item in a.kernel_stats}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
